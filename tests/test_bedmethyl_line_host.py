"""The bedMethyl readers' host halves (no GPU).

1. The grammar of a line, mkp_bedmethyl_parse_line (modkit_amd/csrc/mkp_bedmethyl_line.hpp) — the one copy the host reader and the device
   reader's parse kernel share: tests/bedmethyl_line_host.cpp is compiled with g++ alone (with -fsanitize=address,undefined when g++'s
   sanitizer runtime is installed; each line is handed over as a heap copy of exactly its bytes) and run on every READER and BAD text of
   tests/test_bedmethyl_merge_host.py and on 2 000 seeded lines, each valid or with exactly one defect.  A valid line must give what the
   model's parse_line gives (tests/bedmethyl_merge_model.py); a defect must give its status class and field, worked out by the generator.
2. The host reader (mkp_host_read_bedmethyl) on BGZF: files written here with zlib (raw deflate + the 18-byte BGZF header, block cuts
   chosen here: inside lines, empty blocks, with and without the EOF block) and the two bgzip tables of the reference's dmr test equal the
   model on the inflated text; a damaged block, a truncated block and a plain gzip stream are refused with their statuses."""
import gzip
import os
import random
import subprocess

import pytest

import modkit_amd
import bedmethyl_merge_model as model
from bedmethyl_in_cases import (BAD, BAD_PREFIX, IO, LUNG, READER, UNSUPPORTED, bgzf_bytes, model_runs, random_cuts, random_file, random_line,
                                runs_as_records)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def parse_lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("bedmethyl_line_host")
    base = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "modkit_amd", "csrc")]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        san = []   # no sanitizer runtime on this machine: the same checks without it
    exe = d / "bedmethyl_line_host"
    subprocess.check_call(base + san + ["-o", str(exe), os.path.join(ROOT, "tests", "bedmethyl_line_host.cpp")])
    count = [0]

    def run(lines):
        """lines (no '\\n' inside) -> per line ("ok", chrom, start, code text, strand, [8 counts]) or ("err", class, field)"""
        count[0] += 1
        path = d / ("lines%d.txt" % count[0])
        path.write_bytes("".join(l + "\n" for l in lines).encode())
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("MKP_")}
        p = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        out = []
        for ln in p.stdout.splitlines():
            w = ln.split(" ")
            out.append(("err", int(w[1]), int(w[2])) if w[0] == "err" else
                       ("ok", w[1], int(w[2]), model.code_text(int(w[3])), w[4], [int(x) for x in w[5:13]]))
        assert len(out) == len(lines)
        return out
    return run


def expected_ok(l):
    chrom, start, code, strand, counts = model.parse_line(l)
    return ("ok", chrom, start, code, strand, counts)


def test_line_function_on_the_reader_texts(parse_lines):
    lines = [l for case in sorted(READER) for l in READER[case].split("\n") if l and not l.startswith("#")]
    assert len(lines) == 18
    assert parse_lines(lines) == [expected_ok(l) for l in lines]


def test_line_function_on_the_bad_texts(parse_lines):
    cases = sorted(BAD)
    got = parse_lines([BAD[c][0].split("\n")[0] for c in cases])
    assert got == [("err",) + BAD[c][2] for c in cases]


def test_line_function_fuzz(parse_lines):
    r = random.Random(20240611)
    lines, want = [], []
    for _ in range(2000):
        l, defect = random_line(r)
        lines.append(l)
        want.append(expected_ok(l) if defect is None else ("err",) + defect)
    assert sum(w[0] == "ok" for w in want) > 800 and len(set(w[1:] for w in want if w[0] == "err")) > 40
    got = parse_lines(lines)
    for l, g, w in zip(lines, got, want):
        assert g == w, repr(l)


# ---- the host reader on BGZF
def write(tmp_path, data, name):
    p = tmp_path / name
    p.write_bytes(data.encode() if isinstance(data, str) else data)
    return str(p)


@pytest.mark.parametrize("case", sorted(READER))
def test_host_reader_on_bgzf_written_here(tmp_path, case):
    text = READER[case]
    n = len(text)
    layouts = {"one_block": ((), True), "no_eof_block": ((), False), "cut_inside_lines": ((n // 3, n // 2 + 1), True),
               "empty_block_in_the_middle": ((n // 2, n // 2), True), "a_byte_per_block": (tuple(range(1, min(n, 40))), False)}
    for name, (cuts, eof) in layouts.items():
        path = write(tmp_path, bgzf_bytes(text, cuts, eof), name + ".bed.gz")
        assert runs_as_records(modkit_amd.read_bedmethyl_runs(path)) == model_runs(text), name
    assert runs_as_records(modkit_amd.read_bedmethyl_runs(write(tmp_path, text, "plain.bed"))) == model_runs(text)


def test_host_reader_on_seeded_bgzf_files(tmp_path):
    r = random.Random(5)
    for k in range(20):
        text = random_file(r)
        path = write(tmp_path, bgzf_bytes(text, random_cuts(r, len(text)), r.random() < 0.5), "f%d.bed.gz" % k)
        assert runs_as_records(modkit_amd.read_bedmethyl_runs(path)) == model_runs(text)


def test_host_reader_on_the_lung_tables():
    for path, n_lines in zip(LUNG, (17416, 17301)):
        text = gzip.open(path).read().decode()
        want = model_runs(text)
        assert [c for c, _ in want] == ["chr20"] and len(want[0][1]) == n_lines
        assert runs_as_records(modkit_amd.read_bedmethyl_runs(path)) == want


def test_a_bad_line_inside_bgzf_is_named(tmp_path):
    for case in sorted(BAD):
        text, status, _ = BAD[case]
        path = write(tmp_path, bgzf_bytes(BAD_PREFIX + text, (7,)), case + ".bed.gz")
        with pytest.raises(modkit_amd.MkpError) as e:
            modkit_amd.read_bedmethyl_runs(path)
        assert e.value.status == status and "line 3 of " + path in str(e.value), str(e.value)


def test_bgzf_failures_and_their_statuses(tmp_path):
    text = (READER["tabs"] * 40).encode()
    whole = bgzf_bytes(text, (len(text) // 2,))
    second = len(bgzf_bytes(text[:len(text) // 2], eof=False))   # where block 1 starts
    # a flipped byte inside block 1's deflate payload
    damaged = bytearray(whole)
    damaged[second + 18 + 5] ^= 0x5a
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.read_bedmethyl_runs(write(tmp_path, bytes(damaged), "damaged.bed.gz"))
    assert e.value.status == IO and "block 1" in str(e.value), str(e.value)
    # the last block cut short
    no_eof = bgzf_bytes(text, (len(text) // 2,), eof=False)
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.read_bedmethyl_runs(write(tmp_path, no_eof[:-9], "truncated.bed.gz"))
    assert e.value.status == IO and "block 1" in str(e.value), str(e.value)
    # a wrong ISIZE / CRC pair is caught by the CRC
    wrong_crc = bytearray(whole)
    wrong_crc[second - 8] ^= 1   # block 0's CRC-32
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.read_bedmethyl_runs(write(tmp_path, bytes(wrong_crc), "crc.bed.gz"))
    assert e.value.status == IO and "block 0" in str(e.value), str(e.value)
    # gzip without BGZF blocks stays refused
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.read_bedmethyl_runs(write(tmp_path, gzip.compress(text), "plain_gzip.bed.gz"))
    assert e.value.status == UNSUPPORTED and "plain text" in str(e.value)
