"""Host halves of localize (`modkit localize`): the tolerant regions loader (mkp_host_parse_localize_regions), the genome sizes
(mkp_host_parse_genome_sizes), the table writer (mkp_host_localize_table) and the driver's argument refusals against the independent model
of tests/localize_model.py — and that model against the reference's own golden bedMethyl with totals added up by hand here (the reference
has no golden for this command).  No device is needed."""
import os

import numpy as np
import pytest

import modkit_amd
import localize_model as model
from pileup_cases import FIX

GOLDEN = os.path.join(FIX, "modbam.modpileup_nofilt.methyl.bed")
BC = os.path.join(FIX, "bc_anchored_10_reads.sorted.bam")
CONTIGS = ["chr1", "chr2", "oligo_1512_adapters"]

BEDS = {
    "bed3": ("chr1\t10\t20\nchr2\t0\t5\nchrX\t7\t9\n", 0),
    "bed4_name_with_blanks": ("chr1\t10\t20\tisland\nchr2\t0\t5\ta b\nchr1\t3\t4\n", 0),
    # three tab fields but six whitespace fields in the first line: `stats` would take the bed3/4 parser, localize takes the stranded one,
    # which the bed3 line at the end then fails
    "whitespace_not_tab_fields": ("chr1 10 20 island\t0\t+\nchr2\t0\t5\tb\t0\t-\nchr1\t3\t4\n", 1),
    "blank_separated_stranded": ("chr1 10 20 n\t0 +\nchr2 0 5 m\t. -\n", 0),   # (a name ends at a tab only: it may hold blanks)
    "bad_lines_among_good": ("chr1\t10\t20\nnot a line\n\nchr2\tx\t5\nchr2\t0\t5\nchr1\t7\n", 4),
    "comment_lines": ("#chrom\tstart\tend\nchr1\t1\t2\n# note\nchr2\t3\t4\n", 2),   # a '#' line goes through the parser too, and fails it
    "stranded_with_a_bed3_line": ("chr1\t1\t2\tn\t0\t+\nchr1\t3\t4\nchr2\t5\t6\tm\t1.5\t-\nchr2\t5\t6\tm\tabc\t-\n", 2),
    "first_line_decides_unstranded": ("chr1\t1\t2\tn\nchr1\t3\t4\tm\t0\t-\n", 0),
    "start_after_end": ("chr1\t9\t3\nchr2\t5\t5\n", 0),
    "no_final_newline_crlf": ("chr1\t1\t2\r\nchr2\t3\t4", 0),
    "empty_first_line": ("\nchr1\t1\t2\tn\t0\t-\n", 1),   # the empty line has no field: bed3/4 parser, which it then fails itself
}
REFUSED = {
    "empty": "",
    "only_comments": "#a\n#b\n",
    "all_bad": "chr1\t1\nfoo\n\n",
    "all_bad_for_the_stranded_parser": "chr1\t1\t2\tn\t0\tx\nchr1\t3\t4\n",
}


def write(tmp_path, text, name="r.bed"):
    p = tmp_path / name
    p.write_bytes(text.encode())
    return str(p)


@pytest.mark.parametrize("case", sorted(BEDS))
def test_loader_equals_the_model(tmp_path, case):
    text, skipped = BEDS[case]
    want, want_skipped = model.parse_regions(text)
    assert want_skipped == skipped   # (pinned by hand above, so that two equal mistakes do not pass)
    rs = modkit_amd.RegionSet(write(tmp_path, text), CONTIGS, localize=True)
    assert [(c, s, e, st) for c, s, e, _n, st in rs.regions] == want
    assert rs.skipped == skipped
    assert rs.tids == [CONTIGS.index(c) if c in CONTIGS else -1 for c, *_ in want]
    rs.close()


def test_loader_pins():
    assert model.parse_regions(BEDS["whitespace_not_tab_fields"][0])[0] == [("chr1", 10, 20, "+"), ("chr2", 0, 5, "-")]
    assert model.parse_regions(BEDS["stranded_with_a_bed3_line"][0])[0] == [("chr1", 1, 2, "+"), ("chr2", 5, 6, "-")]
    assert model.parse_regions(BEDS["first_line_decides_unstranded"][0])[0][1] == ("chr1", 3, 4, ".")
    assert model.parse_regions(BEDS["start_after_end"][0])[0][0] == ("chr1", 9, 3, ".")
    assert model.parse_regions(BEDS["bad_lines_among_good"][0])[0] == [("chr1", 10, 20, "."), ("chr2", 0, 5, ".")]


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_loader_fails_only_when_no_line_parsed(tmp_path, case):
    with pytest.raises(model.LocalizeError):
        model.parse_regions(REFUSED[case])
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.RegionSet(write(tmp_path, REFUSED[case]), CONTIGS, localize=True)
    assert e.value.status == -1   # MKP_E_INVALID


# ---- genome sizes
def test_sizes_parser(tmp_path):
    text = "chr1\t1000\nchr2 2000 trailing words\nchr3\t \t7\r\nchr1\t1500\n"
    assert model.parse_sizes(text) == {"chr1": 1500, "chr2": 2000, "chr3": 7}
    got = modkit_amd.genome_sizes(write(tmp_path, text, "g.sizes"))
    assert dict(got) == model.parse_sizes(text) and [n for n, _ in got] == ["chr1", "chr2", "chr3"]   # the later duplicate holds, at the first's place
    assert modkit_amd.genome_sizes(write(tmp_path, "", "empty.sizes")) == []
    for bad in ["chr1\t1000\n\nchr2\t5\n", "chr1\n", "chr1\tx\n", "#name\tlength\n"]:
        with pytest.raises(model.LocalizeError):
            model.parse_sizes(bad)
        with pytest.raises(modkit_amd.MkpError) as e:
            modkit_amd.genome_sizes(write(tmp_path, bad, "bad.sizes"))
        assert e.value.status == -1


# ---- the table writer: hand-built counts
TABLE_COUNTS = {"m": {-3: [0, 7], 0: [3, 3], 2: [1, 3]}, "h": {-1: [5000000000, 15000000000], 3: [0, 0]}, "21839": {1: [2, 3]}, "a": {-3: [9, 9]}}


def counts_for(counts, window):
    cols = sorted(counts, key=model.code_key)
    shape = (len(cols), 2 * window + 1)
    out = {"codes": [modkit_amd.code_repr(c) for c in cols], "window": window, "n_mod": np.zeros(shape, dtype=np.uint64),
           "n_valid": np.zeros(shape, dtype=np.uint64), "n_rows": np.zeros(shape, dtype=np.uint64)}
    for k, c in enumerate(cols):
        for off, (n_mod, n_valid) in counts[c].items():
            out["n_mod"][k, off + window], out["n_valid"][k, off + window], out["n_rows"][k, off + window] = n_mod, n_valid, 1
    return out


@pytest.mark.parametrize("counts,window", [(TABLE_COUNTS, 3), (TABLE_COUNTS, 40), ({"m": {0: [1, 2]}}, 0), ({}, 5)], ids=["w3", "w40", "w0", "empty"])
def test_table_writer_equals_the_model(tmp_path, counts, window):
    out = str(tmp_path / "t.tsv")
    modkit_amd.write_localize_table(counts_for(counts, window), out)
    assert open(out).read() == model.format_table(counts)


def test_table_pins():
    """codes in ModCodeRepr order (letters, then ChEBI numbers), offsets ascending, a zero-coverage cell, percentages through f32 Display"""
    assert model.format_table(TABLE_COUNTS).split("\n") == [
        "mod_code\toffset\tn_valid\tn_mod\tpercent_modified",
        "a\t-3\t9\t9\t100",
        # (15 000 000 000 is no f32: `as f32` rounds it to 15 000 000 512, so this third comes out one step lower than 1 / 3 does)
        "h\t-1\t15000000000\t5000000000\t33.333332",
        "h\t3\t0\t0\t0",
        "m\t-3\t7\t0\t0",
        "m\t0\t3\t3\t100",
        "m\t2\t3\t1\t33.333336",
        "21839\t1\t3\t2\t66.66667",
        ""]
    assert model.format_table({}) == "mod_code\toffset\tn_valid\tn_mod\tpercent_modified\n"


# ---- the model on the reference's data, totals added up by hand from the golden lines (window 3, the contig taken as 147 long)
CONTIG = "oligo_1512_adapters"
GOLDEN_SIZES = CONTIG + "\t147\nelsewhere\t1000\n"
GOLDEN_BED = (CONTIG + "\t62\t66\n"       # A: mp 64, window [60, 67), anchor 63: rows at 63 (+ and -), 64, 65 -> offsets 0, -1, -2; 8 lines
              + CONTIG + "\t91\t96\n"     # D: mp 93, window [89, 96), anchor 92: 90 -> +2, 91 -> +1, 93 -> -1, 94 (+ and -) -> -2, 95 -> -3; 12 lines
              + CONTIG + "\t70\t73\n"     # E: mp 71, window [67, 74), anchor 70: 69 -> +1, 70 -> 0, 72 -> -2, 73 -> -3; 8 lines
              + CONTIG + "\t144\t148\n"   # C: mp 146, window [142, min(149, 147)), anchor 144 (not 145): 146 -> -2; 2 lines
              + CONTIG + "\t2\t4\n"       # clipped at 0: mp 3, window [0, 6): no golden line lies there
              + CONTIG + "\t400\t500\n"   # behind the contig end: ws 446 >= we 147, nothing fetched
              + "elsewhere\t60\t70\n"     # in the sizes, not in the bedMethyl: dropped
              + "nowhere\t60\t70\n")      # not in the sizes: dropped
# (n_valid, n_mod) per offset, added up by hand from the lines asserted below
BY_HAND = {
    "h": {-3: (1 + 4, 1 + 0), -2: (2 + 1 + 3 + 6 + 3, 0 + 0 + 3 + 2 + 1), -1: (2 + 4, 1 + 2), 0: (6 + 1 + 4, 1 + 1 + 0), 1: (4 + 5, 4 + 0), 2: (5, 2)},
    "m": {-3: (1 + 4, 0 + 4), -2: (2 + 1 + 3 + 6 + 3, 2 + 1 + 0 + 4 + 0), -1: (2 + 4, 1 + 2), 0: (6 + 1 + 4, 5 + 0 + 4), 1: (4 + 5, 0 + 5), 2: (5, 3)},
}


def cells(table_text):
    """(code, offset, n_valid, n_mod) of every table line"""
    lines = table_text.splitlines()
    assert lines[0] == "mod_code\toffset\tn_valid\tn_mod\tpercent_modified"
    return [(f[0], int(f[1]), int(f[2]), int(f[3])) for f in (l.split("\t") for l in lines[1:])]


def test_model_on_the_golden_bedmethyl():
    text = open(GOLDEN).read()
    rows = [l.split("\t") for l in text.splitlines()]
    def line(pos, code, strand):   # (valid coverage, modified) of one golden line, checked to be there exactly once
        hit = [r for r in rows if r[1] == str(pos) and r[3] == code and r[5] == strand]
        assert len(hit) == 1
        return int(hit[0][9]), int(hit[0][11])
    assert sorted({int(r[1]) for r in rows if 60 <= int(r[1]) < 67}) == [63, 64, 65] and not [r for r in rows if int(r[1]) < 9 or int(r[1]) > 146]
    assert sorted({int(r[1]) for r in rows if 89 <= int(r[1]) < 96}) == [90, 91, 93, 94, 95]
    assert sorted({int(r[1]) for r in rows if 67 <= int(r[1]) < 74}) == [69, 70, 72, 73] and [int(r[1]) for r in rows if int(r[1]) >= 142] == [146, 146]
    # the contributing lines, as read off the golden file
    assert [line(63, "h", "+"), line(63, "h", "-"), line(64, "h", "-"), line(65, "h", "-")] == [(6, 1), (1, 1), (2, 1), (2, 0)]            # A
    assert [line(63, "m", "+"), line(63, "m", "-"), line(64, "m", "-"), line(65, "m", "-")] == [(6, 5), (1, 0), (2, 1), (2, 2)]
    assert [line(90, "h", "+"), line(91, "h", "-"), line(93, "h", "+"), line(94, "h", "+"), line(94, "h", "-"), line(95, "h", "-")] == [
        (5, 2), (4, 4), (4, 2), (1, 0), (3, 3), (1, 1)]                                                                                      # D
    assert [line(90, "m", "+"), line(91, "m", "-"), line(93, "m", "+"), line(94, "m", "+"), line(94, "m", "-"), line(95, "m", "-")] == [
        (5, 3), (4, 0), (4, 2), (1, 1), (3, 0), (1, 0)]
    assert [line(69, "h", "+"), line(70, "h", "-"), line(72, "h", "+"), line(73, "h", "-")] == [(5, 0), (4, 0), (6, 2), (4, 0)]            # E
    assert [line(69, "m", "+"), line(70, "m", "-"), line(72, "m", "+"), line(73, "m", "-")] == [(5, 5), (4, 4), (6, 4), (4, 4)]
    assert [line(146, "h", "-"), line(146, "m", "-")] == [(3, 1), (3, 0)]                                                                    # C
    got = model.localize_table(text, GOLDEN_BED, GOLDEN_SIZES, window=3)
    want = ["mod_code\toffset\tn_valid\tn_mod\tpercent_modified"]
    for code in ("h", "m"):
        for off in sorted(BY_HAND[code]):
            n_valid, n_mod = BY_HAND[code][off]
            want.append("%s\t%d\t%d\t%d\t%s" % (code, off, n_valid, n_mod, model.rust_f32(np.float32(n_mod) / np.float32(n_valid) * np.float32(100))))
    assert got.splitlines() == want and got.endswith("\n")
    assert got.splitlines()[1] == "h\t-3\t5\t1\t20" and "h\t-2\t15\t6\t40" in got.splitlines()
    # the row at a region's own midpoint lands on offset -1: region A alone, position 64
    only_a = cells(model.localize_table(text, CONTIG + "\t62\t66\n", GOLDEN_SIZES, window=3))
    assert only_a == [("h", -2, 2, 0), ("h", -1, 2, 1), ("h", 0, 7, 2), ("m", -2, 2, 2), ("m", -1, 2, 1), ("m", 0, 7, 5)]
    # clipped at 0 with a window that reaches a line: mp 2, window [0, 12), anchor 6 (unclipped it would be 1): position 9 -> offset -3
    assert cells(model.localize_table(text, CONTIG + "\t0\t4\n", GOLDEN_SIZES, window=10)) == [("h", -3, 4, 2), ("m", -3, 4, 1)]
    # clipped at the contig end: C alone; with a longer contig the anchor moves back to mp - 1
    assert cells(model.localize_table(text, CONTIG + "\t144\t148\n", GOLDEN_SIZES, window=3)) == [("h", -2, 3, 1), ("m", -2, 3, 0)]
    assert cells(model.localize_table(text, CONTIG + "\t144\t148\n", CONTIG + "\t1512\n", window=3)) == [("h", -1, 3, 1), ("m", -1, 3, 0)]
    # strands: region A as a '-' feature fetches the '-' rows only; --stranded-features + fetches the '+' rows of 63, which `same` then
    # drops ('-' does not overlap '+') and `opposite` keeps; a '.' region keeps nothing under `opposite`
    minus = CONTIG + "\t62\t66\ta\t0\t-\n"
    assert cells(model.localize_table(text, minus, GOLDEN_SIZES, window=3)) == [("h", -2, 2, 0), ("h", -1, 2, 1), ("h", 0, 1, 1), ("m", -2, 2, 2), ("m", -1, 2, 1), ("m", 0, 1, 0)]
    assert cells(model.localize_table(text, minus, GOLDEN_SIZES, window=3, stranded="same", stranded_features="+")) == []
    assert cells(model.localize_table(text, minus, GOLDEN_SIZES, window=3, stranded="opposite", stranded_features="+")) == [("h", 0, 6, 1), ("m", 0, 6, 5)]
    assert cells(model.localize_table(text, CONTIG + "\t62\t66\n", GOLDEN_SIZES, window=3, stranded="opposite")) == []
    # no region left: the run fails
    for bed in ["elsewhere\t60\t70\n", "nowhere\t60\t70\n"]:
        with pytest.raises(model.LocalizeError):
            model.localize_table(text, bed, GOLDEN_SIZES, window=3)


# ---- the driver's argument refusals (before any device is touched)
def test_driver_refuses_bad_flag_combinations(tmp_path):
    bed = write(tmp_path, "oligo_1512_adapters\t62\t66\n")
    out, table = str(tmp_path / "o.bed"), str(tmp_path / "t.tsv")
    loc = ["--localize", bed, "--localize-out", table]
    def refused(argv, status, word, hemi=False):
        with pytest.raises(modkit_amd.MkpError) as e:
            (modkit_amd.pileup_hemi if hemi else modkit_amd.pileup)(argv)
        assert e.value.status == status and word in str(e.value), (argv, str(e.value))
    base = [BC, out, "--no-filtering"]
    refused(base + loc + ["--partition-tag", "HP"], -1, "--partition-tag")
    refused(base + loc + ["--gpus-world", "2", "--gpus-rank", "0"], -3, "--gpus-world")
    refused(base + loc + ["--plan-only"], -1, "--plan-only")
    refused(base + loc + ["--localize-only", "--bgzf"], -1, "--localize-only")
    refused(base + loc + ["--localize-only", "--bedgraph"], -1, "--localize-only")
    refused(base + ["--localize", bed], -1, "--localize-out")
    for dependent in (["--localize-out", table], ["--localize-window", "5"], ["--localize-stranded", "same"], ["--localize-stranded-features", "+"],
                      ["--localize-only"]):
        refused(base + dependent, -1, "need --localize")
    refused(base + loc + ["--localize-stranded", "both"], -1, "same or opposite")
    refused(base + loc + ["--localize-stranded-features", "x"], -1, "--localize-stranded-features")
    refused(base + loc + ["--localize-window", "-3"], -1, "--localize-window")
    refused(base + loc + ["--localize-window", "100001"], -3, "--localize-window")
    refused([os.path.join(FIX, "duplex_modcalls_sort.bam"), "-o", out, "--cpg", "--ref", os.path.join(FIX, "CGI_ladder_3.6kb_ref.fa")] + loc, -1,
            "unexpected argument '--localize'", hemi=True)
    assert not os.path.exists(table) and not os.path.exists(out)
