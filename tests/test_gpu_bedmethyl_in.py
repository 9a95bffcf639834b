"""The device bedMethyl reader (modkit_amd/csrc/mkp_bedmethyl.hip behind mkp_bedmethyl_read_device and mkp_merge_add_file): BGZF or plain
bedMethyl text is inflated, cut into lines and parsed in HBM.  Everything is compared with the host reader (the CPU path, which
tests/test_bedmethyl_line_host.py pins to the model) and with the model of tests/bedmethyl_merge_model.py itself.
1. Context.read_bedmethyl_runs == read_bedmethyl_runs == model on the READER texts (plain and BGZF) and the two bgzip tables of the
   reference's dmr test;  2. line ends, '#' lines and long lines on the edges of the line kernels' chunks (C = mkp_bedmethyl_chunk_bytes());
3. piece seams, in a child process with MKP_BEDMETHYL_PIECE_KB=64 (tests/bedmethyl_in_seams.py);  4. failures: every BAD text with the host
   reader's status and message, a pos that descends inside a run, a damaged BGZF block;  5. a seeded fuzz of 100 files, device rows == host
   rows bit for bit;  6. the commands: `bedmethyl merge` and `pileup --merge-bedmethyl` on bgzip tables against the model and against the host
   route (MKP_HOST_BEDMETHYL=1).
Every test here fails on the commit before the reader: from a missing symbol, or from the refusal of gzip input."""
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import modkit_amd
import bedmethyl_merge_model as model
from bedmethyl_in_cases import (BAD, BAD_PREFIX, CHR20_LENGTH, FIX, INVALID, IO, LUNG, READER, UNSUPPORTED, bgzf_bytes, line, model_runs, random_cuts,
                                random_file, runs_as_records)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("pos", "strand", "code_repr", "motif_idx") + model.COUNTS


@pytest.fixture(scope="module")
def ctx():
    c = modkit_amd.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def C():
    return modkit_amd.bedmethyl_chunk_bytes()


def write(tmp_path, data, name):
    p = tmp_path / name
    p.write_bytes(data.encode() if isinstance(data, str) else data)
    return str(p)


def same_bits(dev, host):
    """the runs of the two readers: the same chroms and, column by column, the same arrays"""
    assert [c for c, _ in dev] == [c for c, _ in host]
    for (_, a), (_, b) in zip(dev, host):
        for f in FIELDS:
            assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), f


def check(ctx, path, text):
    dev, host = ctx.read_bedmethyl_runs(path), modkit_amd.read_bedmethyl_runs(path)
    same_bits(dev, host)
    assert runs_as_records(dev) == model_runs(text)
    return dev


# ---- 1. the reader's texts and the reference's tables
@pytest.mark.parametrize("case", sorted(READER))
def test_reader_texts_plain_and_bgzf(ctx, tmp_path, case):
    text = READER[case]
    n = len(text)
    dev = check(ctx, write(tmp_path, text, "plain.bed"), text)
    for name, (cuts, eof) in {"one_block": ((), True), "no_eof_block": ((), False), "cut_inside_lines": ((n // 3, n // 2 + 1), True),
                              "empty_block_in_the_middle": ((n // 2, n // 2), True)}.items():
        check(ctx, write(tmp_path, bgzf_bytes(text, cuts, eof), name + ".bed.gz"), text)
    if case == "contig_runs":
        assert [c for c, _ in dev] == ["c1", "c2", "c1"]
    if case == "empty":
        assert dev == []


def test_the_lung_tables(ctx):
    for path, n_lines in zip(LUNG, (17416, 17301)):
        dev = check(ctx, path, gzip.open(path).read().decode())
        assert [c for c, _ in dev] == ["chr20"] and len(dev[0][1]["pos"]) == n_lines


# ---- 2. chunk edges
def sized(n_bytes, start, chrom="c", end="\n"):
    """a data line of exactly n_bytes (its line end included), sized by its chrom name"""
    body = line(chrom, start, "m", "+", [3, 1, 1, 1, 0, 0, 0, 0])[:-1]
    out = line(chrom + "x" * (n_bytes - len(body) - len(end)), start, "m", "+", [3, 1, 1, 1, 0, 0, 0, 0])[:-1] + end
    assert len(out) == n_bytes
    return out


def comment(n_bytes):
    return "#" + "y" * (n_bytes - 2) + "\n"


def test_chunk_edges(ctx, tmp_path, C):
    few = "".join(sized(70, 10 * k) for k in range(5))                 # 350 bytes of data lines
    after = "".join(sized(70, 1000 + 10 * k) for k in range(5))
    texts = {
        "newline_is_the_last_byte_of_a_chunk": few + sized(C - len(few), 500) + after,
        "newline_is_the_first_byte_of_a_chunk": few + sized(C - len(few) + 1, 500) + after,
        "comment_ends_a_chunk_and_data_begins_the_next": few + comment(C - len(few)) + after,
        "comment_begins_exactly_at_a_chunk_start": few + sized(C - len(few), 500) + comment(33) + after,
        "comment_newline_is_the_first_byte_of_a_chunk": few + comment(C - len(few) + 1) + after,
        "crlf_straddles_a_chunk_seam": few + sized(C - len(few) + 1, 500, end="\r\n") + after,
        "a_data_line_spans_three_chunks": few + sized(2 * C + 200, 500) + after,
        "a_comment_spans_three_chunks": few + comment(2 * C + 200) + after,
        "size_C_minus_1": few + sized(C - 1 - len(few), 500),
        "size_C": few + sized(C - len(few), 500),
        "size_C_plus_1": few + sized(C + 1 - len(few), 500),
        "size_C_without_final_newline": few + sized(C - len(few) + 1, 500)[:-1],
        "size_C_plus_1_without_final_newline": few + sized(C - len(few) + 2, 500)[:-1],
        "last_line_starts_a_chunk_and_has_no_newline": few + sized(C - len(few), 500) + sized(70, 600)[:-1],
        "one_byte_lines_of_comments": few + "#\n" * (C // 2) + after,
        "comments_only": comment(40) + "#\n" + comment(C),
        "comments_only_no_final_newline": comment(40) + "# the end",
        "one_line_without_final_newline": sized(70, 5)[:-1],
        "one_line": sized(70, 5),
        "empty": "",
        "five_chunks_of_short_lines": "".join(sized(60 + k % 9, 3 * k) for k in range(5 * C // 64)),
    }
    assert texts["newline_is_the_last_byte_of_a_chunk"][C - 1] == "\n" and texts["newline_is_the_first_byte_of_a_chunk"][C] == "\n"
    assert texts["comment_begins_exactly_at_a_chunk_start"][C - 1:C + 1] == "\n#"
    assert texts["crlf_straddles_a_chunk_seam"][C - 1:C + 1] == "\r\n"
    assert [len(texts["size_C" + s]) for s in ("_minus_1", "", "_plus_1")] == [C - 1, C, C + 1]
    for name in sorted(texts):
        text = texts[name]
        dev = check(ctx, write(tmp_path, text, name + ".bed"), text)
        check(ctx, write(tmp_path, bgzf_bytes(text, (C, 2 * C + 1) if len(text) > C else ()), name + ".bed.gz"), text)
        if name.startswith("comments_only") or name == "empty":
            assert dev == []


# ---- 3. piece seams
def test_piece_seams_in_a_child_process():
    env = dict(os.environ, MKP_BEDMETHYL_PIECE_KB="64", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    p = subprocess.run([sys.executable, os.path.join(HERE, "bedmethyl_in_seams.py")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-300:], p.stderr[-2000:])
    assert int(p.stdout.split()[1]) >= 25


# ---- 4. failures
@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_line_has_the_host_readers_status_and_message(ctx, tmp_path, case):
    text, status, _ = BAD[case]
    for name, data in (("in.bed", BAD_PREFIX + text), ("in.bed.gz", bgzf_bytes(BAD_PREFIX + text, (9,)))):
        path = write(tmp_path, data, name)
        with pytest.raises(modkit_amd.MkpError) as host:
            modkit_amd.read_bedmethyl_runs(path)
        with pytest.raises(modkit_amd.MkpError) as dev:
            ctx.read_bedmethyl_runs(path)
        assert dev.value.status == host.value.status == status and str(dev.value) == str(host.value), (str(dev.value), str(host.value))
        assert "line 3 of " + path in str(dev.value)
        ctx.merge_begin([100])
        with pytest.raises(modkit_amd.MkpError) as add:
            ctx.merge_add_file(path, ["c1"])
        assert str(add.value) == str(host.value)


def test_descending_pos_inside_a_run_is_invalid(ctx, tmp_path):
    rows = [line("c1", 5, "m", "+", [1] * 8), "# between\n", line("c1", 9, "m", "+", [1] * 8), line("c1", 8, "h", "-", [1] * 8), line("c2", 1, "m", "+", [1] * 8)]
    for name, data in (("in.bed", "".join(rows)), ("in.bed.gz", bgzf_bytes("".join(rows), (30,)))):
        path = write(tmp_path, data, name)
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.read_bedmethyl_runs(path)
        assert e.value.status == INVALID and "ascending" in str(e.value) and "line 4 of " + path in str(e.value), str(e.value)
    rows[3] = line("c1", 9, "h", "-", [1] * 8)          # equal positions are in order
    check(ctx, write(tmp_path, "".join(rows), "ok.bed"), "".join(rows))


def test_a_damaged_bgzf_block_is_named(ctx, tmp_path):
    text = READER["tabs"] * 60
    half = len(text) // 2
    whole = bgzf_bytes(text, (half,))
    second = len(bgzf_bytes(text[:half], eof=False))    # where block 1 starts
    damaged = bytearray(whole); damaged[second + 18 + 5] ^= 0x5a
    wrong_crc = bytearray(whole); wrong_crc[second - 8] ^= 1
    for name, data, word in (("damaged", bytes(damaged), "block 1"), ("wrong_crc", bytes(wrong_crc), "block 0"),
                             ("truncated", bgzf_bytes(text, (half,), eof=False)[:-9], "block 1")):
        path = write(tmp_path, data, name + ".bed.gz")
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.read_bedmethyl_runs(path)
        assert e.value.status == IO and word in str(e.value), (name, str(e.value))
    with pytest.raises(modkit_amd.MkpError) as e:       # gzip without BGZF blocks stays refused
        ctx.read_bedmethyl_runs(write(tmp_path, gzip.compress(text.encode()), "gzip.bed.gz"))
    assert e.value.status == UNSUPPORTED and "plain text" in str(e.value)
    with pytest.raises(modkit_amd.MkpError) as e:
        ctx.read_bedmethyl_runs(str(tmp_path / "absent.bed"))
    assert e.value.status == IO
    check(ctx, write(tmp_path, whole, "whole.bed.gz"), text)   # the context reads on


# ---- 5. fuzz
def test_seeded_fuzz_device_rows_equal_host_rows(ctx, tmp_path):
    r = random.Random(4711)
    n_rows = n_runs = 0
    for k in range(100):
        text = random_file(r)
        data = text if k % 3 == 0 else bgzf_bytes(text, random_cuts(r, len(text)), eof=r.random() < 0.5)
        path = write(tmp_path, data, "f%d.bed" % k)
        dev, host = ctx.read_bedmethyl_runs(path), modkit_amd.read_bedmethyl_runs(path)
        same_bits(dev, host)
        n_runs += len(dev); n_rows += sum(len(rows["pos"]) for _, rows in dev)
        if k % 10 == 0:
            assert runs_as_records(dev) == model_runs(text)
    assert n_rows > 10000 and n_runs > 300


# ---- 6. the commands
def run_with_env(env, fn, *args):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn(*args)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def test_bedmethyl_merge_on_the_lung_tables(tmp_path):
    sizes_text = "chr19\t58617616\nchr20\t%d\n" % CHR20_LENGTH
    sizes = write(tmp_path, sizes_text, "g.sizes")
    texts = [gzip.open(p).read().decode() for p in LUNG]
    want, want_dropped = model.merge_texts(texts, sizes_text)
    assert want_dropped == 0 and len(want.splitlines()) > 17416
    out = str(tmp_path / "out.bed")
    assert modkit_amd.bedmethyl_merge(LUNG + ["-g", sizes, "-o", out]) == (len(want.splitlines()), 0)
    assert open(out).read() == want
    host = str(tmp_path / "host.bed")
    run_with_env({"MKP_HOST_BEDMETHYL": "1"}, modkit_amd.bedmethyl_merge, LUNG + ["-g", sizes, "-o", host])
    assert open(host, "rb").read() == open(out, "rb").read()
    # a mixed list: one plain, one bgzip
    plain = write(tmp_path, texts[0], "normal.bed")
    mixed = str(tmp_path / "mixed.bed")
    modkit_amd.bedmethyl_merge([plain, LUNG[1], "-g", sizes, "-o", mixed])
    assert open(mixed).read() == want
    # round trip: the command's own --bgzf output is input to the next merge
    third = "".join(line("chr20", 60000 + 7 * k, "m", "+-"[k % 2], [5, 2, 3, 0, 1, 0, 0, 1]) for k in range(500)) + line("chrX", 1, "m", "+", [1] * 8)
    first = str(tmp_path / "first.bed.gz")
    modkit_amd.bedmethyl_merge(LUNG + ["-g", sizes, "-o", first, "--bgzf"])
    again = str(tmp_path / "again.bed")
    n, dropped = modkit_amd.bedmethyl_merge([first, write(tmp_path, third, "third.bed"), "-g", sizes, "-o", again])
    want3, dropped3 = model.merge_texts(texts + [third], sizes_text)
    assert open(again).read() == want3 and (n, dropped) == (len(want3.splitlines()), dropped3) and dropped3 == 1


def test_pileup_merge_bedmethyl_takes_a_bgzip_prior(tmp_path):
    bam = os.path.join(FIX, "bc_anchored_10_reads.sorted.bam")
    flags = ["--no-filtering", "-i", "25"]
    plain_out = str(tmp_path / "plain.bed")
    modkit_amd.pileup([bam, plain_out] + flags)
    lines = open(plain_out).read().splitlines()
    prior_text = "#a prior table\n" + "".join(l + "\n" for k, l in enumerate(lines) if k % 3 == 0) + line("no_such_contig", 5, "m", "+", [4] * 8)
    prior, prior_gz = write(tmp_path, prior_text, "prior.bed"), write(tmp_path, bgzf_bytes(prior_text, (len(prior_text) // 2,)), "prior.bed.gz")
    outs = []
    for k, (p, env) in enumerate(((prior, {}), (prior_gz, {}), (prior_gz, {"MKP_HOST_BEDMETHYL": "1"}))):
        out = str(tmp_path / ("merged%d.bed" % k))
        run_with_env(env, modkit_amd.pileup, [bam, out] + flags + ["--merge-bedmethyl", p])
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] == outs[2] and len(outs[0].splitlines()) == len(lines)
    joined = [l.split("\t") for l in outs[0].decode().splitlines()]
    assert any(int(a[4]) == 2 * int(b.split("\t")[4]) for a, b in zip(joined, lines))   # rows of the prior were summed in
