"""Host halves of `bedmethyl merge`: the plain-text bedMethyl reader (mkp_host_read_bedmethyl) against the independent model of
tests/bedmethyl_merge_model.py, the driver's argument refusals that need no device — and that model against the reference's own golden
bedMethyl files with sums added up by hand here (the reference's only test of this command is the self-merge property, which is run too).
No device is needed."""
import os

import numpy as np
import pytest

import modkit_amd
import bedmethyl_merge_model as model
from pileup_cases import FIX

NOFILT = os.path.join(FIX, "modbam.modpileup_nofilt.methyl.bed")
FILT = os.path.join(FIX, "modbam.modpileup_filt025.methyl.bed")
TWO_MOTIFS = os.path.join(FIX, "cgcg2_cg0_test1.bed")
IO, UNSUPPORTED, INVALID = -2, -3, -1


def line(chrom, start, name, strand, counts, sep="\t", tail_sep=None):
    """one bedMethyl line; counts = [valid, mod, canonical, other, delete, fail, diff, nocall]"""
    tail_sep = sep if tail_sep is None else tail_sep
    head = sep.join([chrom, str(start), str(start + 1), name, str(counts[0]), strand, str(start), str(start + 1), "255,0,0"])
    return head + sep + tail_sep.join([str(counts[0]), "12.50"] + [str(c) for c in counts[1:]]) + "\n"


def write(tmp_path, text, name="in.bed"):
    p = tmp_path / name
    p.write_bytes(text.encode() if isinstance(text, str) else text)
    return str(p)


def runs_as_records(runs):
    return [(chrom, model.records_of_rows(rows)) for chrom, rows in runs]


def model_runs(text):
    out = []
    for l in text.splitlines():
        if l.startswith("#"):
            continue
        chrom, start, code, strand, counts = model.parse_line(l)
        if not out or out[-1][0] != chrom:
            out.append((chrom, []))
        out[-1][1].append((start, code, strand, counts))
    return out


# ---- the reader
READER = {
    "tabs": line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7]) + line("c1", 5, "h", "-", [8, 7, 6, 5, 4, 3, 2, 1]),
    "mixed_delim": line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7], tail_sep=" ") + line("c1", 6, "a", ".", [1, 1, 0, 0, 0, 0, 0, 0], sep=" "),
    "chebi_and_motif_names": line("c1", 5, "21839", "+", [9, 1, 2, 3, 4, 5, 6, 7]) + line("c1", 5, "m,CG,0", "+", [3, 1, 1, 1, 0, 0, 0, 0])
                             + line("c1", 5, "m,CGCG,2", "+", [3, 1, 1, 1, 0, 0, 0, 0]) + line("c1", 9, "76792,A,0", "-", [2, 2, 0, 0, 0, 0, 0, 0]),
    "comment_lines": "#chrom\tstart\n" + line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7]) + "# a note\n" + line("c2", 1, "m", "-", [1, 0, 1, 0, 0, 0, 0, 0]),
    "contig_runs": line("c1", 5, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0]) + line("c2", 1, "m", "+", [2, 1, 0, 0, 0, 0, 0, 0])
                   + line("c2", 4, "m", "+", [3, 1, 0, 0, 0, 0, 0, 0]) + line("c1", 2, "m", "+", [4, 1, 0, 0, 0, 0, 0, 0]),
    "no_final_newline_crlf": line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7]).replace("\n", "\r\n") + line("c1", 6, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0])[:-1],
    "large_counts": line("c1", 4000000000, "m", "+", [4294967295, 4294967295, 0, 0, 0, 0, 0, 4294967295]),
    "the_score_is_the_coverage": "c1\t5\t6\tm\t9\t+\t5\t6\t255,0,0\t77\t1.00\t1\t2\t3\t4\t5\t6\t7\n",
    "empty": "",
}


@pytest.mark.parametrize("case", sorted(READER))
def test_reader_equals_the_model(tmp_path, case):
    text = READER[case]
    got = modkit_amd.read_bedmethyl_runs(write(tmp_path, text))
    assert runs_as_records(got) == model_runs(text)
    for _chrom, rows in got:
        assert (rows["motif_idx"] == -1).all()
    if case == "contig_runs":
        assert [c for c, _ in got] == ["c1", "c2", "c1"]
    if case == "the_score_is_the_coverage":
        assert int(got[0][1]["n_valid"][0]) == 9
    if case == "chebi_and_motif_names":
        assert list(got[0][1]["code_repr"]) == [21839 | 1 << 31, ord("m"), ord("m"), 76792 | 1 << 31]
    if case == "empty":
        assert got == []


def test_reader_reads_the_golden_files():
    for path in (NOFILT, FILT, TWO_MOTIFS):
        text = open(path).read()
        assert runs_as_records(modkit_amd.read_bedmethyl_runs(path)) == model_runs(text)


BAD = {
    "too_few_fields": ("c1\t5\t6\tm\t9\t+\t5\t6\t255,0,0\t9\t1.00\t1\t2\t3\t4\t5\t6\n", IO),
    "count_not_a_number": (line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7]).replace("\t7\n", "\tx\n"), IO),
    "bad_strand": (line("c1", 5, "m", "*", [9, 1, 2, 3, 4, 5, 6, 7]), IO),
    "bad_code": (line("c1", 5, "mh", "+", [9, 1, 2, 3, 4, 5, 6, 7]), IO),
    "blank_line_between": ("\n" + line("c1", 6, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0]), IO),
    "count_beyond_32_bits": (line("c1", 5, "m", "+", [4294967296, 1, 0, 0, 0, 0, 0, 0]), UNSUPPORTED),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_line_fails_the_file_and_is_named(tmp_path, case):
    text, status = BAD[case]
    path = write(tmp_path, line("c1", 1, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0]) + "# skipped, still counted as a line\n" + text)
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.read_bedmethyl_runs(path)
    assert e.value.status == status and "line 3 of " + path in str(e.value), str(e.value)


def test_gzip_magic_and_missing_file_are_refused(tmp_path):
    import gzip
    path = write(tmp_path, gzip.compress(READER["tabs"].encode()), "in.bed.gz")
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.read_bedmethyl_runs(path)
    assert e.value.status == UNSUPPORTED and "plain text" in str(e.value)
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.read_bedmethyl_runs(str(tmp_path / "absent.bed"))
    assert e.value.status == IO


# ---- refusals that are decided before any device work
def test_argument_refusals(tmp_path):
    a, sizes = write(tmp_path, READER["tabs"], "a.bed"), write(tmp_path, "c1\t100\n", "g.sizes")
    out = str(tmp_path / "out.bed")
    def refused(argv, status, word, run=modkit_amd.bedmethyl_merge):
        with pytest.raises(modkit_amd.MkpError) as e:
            run(argv)
        assert e.value.status == status and word in str(e.value), (argv, str(e.value))
    refused([a, "-g", sizes, "-o", out], INVALID, "usage")
    refused([a, a, "-o", out], INVALID, "-g")
    refused([a, a, "-g", sizes], INVALID, "-o")
    refused([a, a, "-g", sizes, "-o", out, "--mixed-delim"], INVALID, "unexpected argument '--mixed-delim'")
    refused([a, a, "-g", sizes, "-o", out, "--header"], INVALID, "unexpected argument '--header'")
    refused([a, a, "-g", sizes, "-o", "-", "--bgzf"], INVALID, "--bgzf")
    existing = write(tmp_path, "keep me\n", "existing.bed")
    refused([a, a, "-g", sizes, "-o", existing], IO, "--force")
    assert open(existing).read() == "keep me\n"
    refused([a, str(tmp_path / "absent.bed"), "-g", sizes, "-o", out], IO, "absent.bed")
    assert not os.path.exists(out)
    # the fused flag
    bam = os.path.join(FIX, "bc_anchored_10_reads.sorted.bam")
    base = [bam, str(tmp_path / "x.bed"), "--no-filtering", "--merge-bedmethyl", a]
    refused(base + ["--partition-tag", "HP"], INVALID, "--partition-tag", run=modkit_amd.pileup)
    refused(base + ["--bedgraph"], INVALID, "--bedgraph", run=modkit_amd.pileup)
    refused(base + ["--region-stats", a, "--region-stats-out", out], INVALID, "--region-stats", run=modkit_amd.pileup)
    refused(base + ["--localize", a, "--localize-out", out], INVALID, "--localize", run=modkit_amd.pileup)
    refused(base + ["--plan-only"], INVALID, "--plan-only", run=modkit_amd.pileup)
    refused(base + ["--gpus-world", "2", "--gpus-rank", "0"], UNSUPPORTED, "--gpus-world", run=modkit_amd.pileup)
    refused([bam, "-o", str(tmp_path / "h.bed"), "--cpg", "--merge-bedmethyl", a], INVALID, "unexpected argument '--merge-bedmethyl'",
            run=modkit_amd.pileup_hemi)
    refused([bam, str(tmp_path / "x.bed"), "--merge-bedmethyl"], INVALID, "missing value", run=modkit_amd.pileup)


# ---- the model, pinned by sums added up by hand from the golden files
def test_model_on_two_golden_files_sums_added_by_hand():
    merged, dropped = model.merge_texts([open(NOFILT).read(), open(FILT).read()], "oligo_1512_adapters\t1512\n")
    lines = merged.splitlines(keepends=True)
    assert dropped == 0 and len(lines) == 52   # every key of the filtered file is in the unfiltered one, which has 52
    # position 9, 'h', '+': 4 2 1 1 0 0 2 0 and 2 1 0 1 0 2 2 0
    assert "oligo_1512_adapters\t9\t10\th\t6\t+\t9\t10\t255,0,0\t6\t50.00\t3\t1\t2\t0\t2\t4\t0\n" in lines
    # position 9, 'm', '+': 4 1 1 2 0 0 2 0 and 2 1 0 1 0 2 2 0: 2 / 6 = 33.33
    assert "oligo_1512_adapters\t9\t10\tm\t6\t+\t9\t10\t255,0,0\t6\t33.33\t2\t1\t3\t0\t2\t4\t0\n" in lines
    # position 72, 'h', '+': 6 2 0 4 0 0 0 0 and 4 1 0 3 0 2 0 0
    assert "oligo_1512_adapters\t72\t73\th\t10\t+\t72\t73\t255,0,0\t10\t30.00\t3\t0\t7\t0\t2\t0\t0\n" in lines
    # position 83, '-': only the unfiltered file has it; the lines come through as they are
    assert "oligo_1512_adapters\t83\t84\th\t1\t-\t83\t84\t255,0,0\t1\t100.00\t1\t0\t0\t0\t0\t0\t3\n" in lines
    assert "oligo_1512_adapters\t83\t84\tm\t1\t-\t83\t84\t255,0,0\t1\t0.00\t0\t0\t1\t0\t0\t0\t3\n" in lines
    assert not any(l.startswith("oligo_1512_adapters\t83\t") for l in open(FILT))
    keys = [model.sort_key((int(l.split()[1]), l.split()[3], l.split()[5])) for l in lines]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_model_collapses_the_two_names_of_a_multi_motif_run():
    text = open(TWO_MOTIFS).read()
    names = {}
    for l in text.splitlines():
        f = l.split()
        names.setdefault((f[1], f[3].split(",")[0], f[5]), set()).add(f[3])
    assert sum(len(v) == 2 for v in names.values()) == 2 and len(text.splitlines()) == 11   # the file really has two names on one key, twice
    merged, dropped = model.merge_texts([text, text], "oligo_741_adapters\t741\n")
    lines = merged.splitlines(keepends=True)
    assert dropped == 0 and len(lines) == 9
    # position 39, '-': `m,CG,0` and `m,CGCG,2`, 4 4 0 0 0 0 0 0 each, in both inputs
    assert "oligo_741_adapters\t39\t40\tm\t16\t-\t39\t40\t255,0,0\t16\t100.00\t16\t0\t0\t0\t0\t0\t0\n" in lines
    # position 40, '+': two names, 8 5 3 0 0 0 0 0 each, in both inputs: 20 / 32 = 62.50
    assert "oligo_741_adapters\t40\t41\tm\t32\t+\t40\t41\t255,0,0\t32\t62.50\t20\t12\t0\t0\t0\t0\t0\n" in lines
    assert all("," not in l.split("\t")[3] for l in lines)


def test_model_self_merge_keeps_the_lines_and_doubles_the_counts():
    """the reference's own test property (tests/test_bedmethyl_util.rs)"""
    text = open(NOFILT).read()
    merged, _ = model.merge_texts([text, text], "oligo_1512_adapters\t1512\n")
    a, b = text.splitlines(), merged.splitlines()
    assert len(a) == len(b) == 52
    for la, lb in zip(a, b):   # (the golden file is in the merge's order already)
        fa, fb = la.split(), lb.split()
        assert fa[:4] == fb[:4] and fa[5:9] == fb[5:9] and fa[10] == fb[10]
        assert [2 * int(x) for x in [fa[4], fa[9]] + fa[11:]] == [int(x) for x in [fb[4], fb[9]] + fb[11:]]


def test_model_order_percent_text_and_filters():
    chebi, a = line("c1", 5, "21839", "+", [3, 1, 0, 0, 0, 0, 0, 0]), line("c1", 5, "a", "+", [3, 2, 0, 0, 0, 0, 0, 0])
    big = line("c1", 5, "76792", "+", [1, 1, 0, 0, 0, 0, 0, 0])
    dot, minus = line("c1", 5, "Z", ".", [0, 0, 0, 0, 0, 0, 0, 9]), line("c1", 5, "a", "-", [0, 4, 0, 0, 0, 0, 0, 0])
    beyond, unlisted = line("c1", 100, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0]), line("c9", 1, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0])
    other = line("c0", 7, "m", "+", [7, 1, 0, 0, 0, 0, 0, 0])
    merged, dropped = model.merge_texts([dot + a + minus + big + beyond + unlisted, chebi + other], "c0 50\nc1\t100\nc2\t5\n")
    rows = [l.split("\t") for l in merged.splitlines()]
    assert dropped == 2
    assert [(r[0], r[3], r[5]) for r in rows] == [("c0", "m", "+"), ("c1", "a", "+"), ("c1", "21839", "+"), ("c1", "76792", "+"), ("c1", "a", "-"),
                                                   ("c1", "Z", ".")]
    assert [r[10] for r in rows] == ["14.29", "66.67", "33.33", "100.00", "inf", "NaN"]
    assert model.percent_text(1, 3) == "33.33" and model.percent_text(1, 8) == "12.50" and model.percent_text(2**32, 2**33) == "50.00"
