"""Host halves of the region statistics (`modkit stats`): the regions BED parser (mkp_host_parse_regions) and the table writer
(mkp_host_stats_table) against the independent model of tests/region_stats_model.py, and that model against the reference's own golden
bedMethyl with totals added up by hand here.  No device is needed."""
import os

import numpy as np
import pytest

import modkit_amd
import region_stats_model as model
from pileup_cases import FIX

GOLDEN = os.path.join(FIX, "modbam.modpileup_nofilt.methyl.bed")
CONTIGS = ["chr1", "chr2", "oligo_1512_adapters"]

BEDS = {
    "bed3": "chr1\t10\t20\nchr2\t0\t5\nchrX\t7\t9\n",
    "bed4": "chr1\t10\t20\tisland one\nchr2\t0\t5\tb\nchr1\t3\t4\n",   # a name may hold blanks; the third line has none
    "stranded": "chr1\t10\t20\tp\t.\t+\nchr2\t0\t5\tq\t0.5\t-\nchr1\t3\t4\tr\t12\t.\nchr2\t1\t2\ts\t1e3\t+\n",
    "no_final_newline": "chr1\t1\t2\nchr2\t3\t4",
    "blank_separated": "chr1 10 20\nchr2 0 5 name\n",
    "empty_region": "chr1\t5\t5\nchr1\t5\t6\n",
    "first_line_decides_unstranded": "chr1\t1\t2\tn\nchr1\t3\t4\tm\t0\t-\n",   # the six-column line goes through the bed4 parser: both strands
}
REFUSED = {
    "comment_first": "#chrom\tstart\tend\nchr1\t1\t2\n",
    "comment_later": "chr1\t1\t2\n# note\n",
    "empty": "",
    "only_comments": "#a\n#b\n",
    "start_after_end": "chr1\t9\t3\n",
    "blank_line": "chr1\t1\t2\n\nchr1\t3\t4\n",
    "no_end": "chr1\t1\n",
    "bad_strand": "chr1\t1\t2\tn\t0\tx\n",
    "no_score": "chr1\t1\t2\tn\tabc\t+\n",
    "stranded_then_short": "chr1\t1\t2\tn\t0\t+\nchr1\t3\t4\n",
}


def write(tmp_path, text, name="r.bed"):
    p = tmp_path / name
    p.write_bytes(text.encode())
    return str(p)


@pytest.mark.parametrize("case", sorted(BEDS))
def test_parser_equals_the_model(tmp_path, case):
    want = model.parse_regions(BEDS[case])
    rs = modkit_amd.RegionSet(write(tmp_path, BEDS[case]), CONTIGS)
    got = rs.regions
    assert got == [(c, s, e, "." if n is None else n, st) for c, s, e, n, st in want]
    assert rs.tids == [CONTIGS.index(c) if c in CONTIGS else -1 for c, *_ in want]
    rs.close()


def test_parser_pins():
    """what the model itself must say about the forms above (so that two equal mistakes do not pass)"""
    assert model.parse_regions(BEDS["bed4"]) == [("chr1", 10, 20, "island one", "."), ("chr2", 0, 5, "b", "."), ("chr1", 3, 4, None, ".")]
    assert [r[4] for r in model.parse_regions(BEDS["stranded"])] == ["+", "-", ".", "+"]
    assert model.parse_regions(BEDS["first_line_decides_unstranded"])[1] == ("chr1", 3, 4, "m", ".")
    assert model.parse_regions(BEDS["empty_region"])[0][1:3] == (5, 5)


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_parser_refuses_what_the_reference_fails_on(tmp_path, case):
    with pytest.raises(model.RegionsError):
        model.parse_regions(REFUSED[case])
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.RegionSet(write(tmp_path, REFUSED[case]), CONTIGS)
    assert e.value.status == -1   # MKP_E_INVALID


def test_parser_refuses_a_name_that_needs_quoting(tmp_path):
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.RegionSet(write(tmp_path, 'chr1\t1\t2\tsay "hi"\n'), CONTIGS)
    assert e.value.status == -3   # MKP_E_UNSUPPORTED


# ---- the table writer: hand-built counts
TABLE_BED = "chr1\t0\t10\tzero\t0\t+\nchr1\t0\t10\tfull\t0\t-\nchr2\t5\t50\tthird\t.\t.\nchrX\t1\t2\tgone\t0\t+\nchr2\t7\t7\ttwo thirds\t3.5\t.\n"
# per region {code: (n_mod, n_valid)}; None = the contig has no rows
TABLE_TOTALS = [{"m": [0, 7], "21839": [3, 3]}, {"m": [9, 9]}, {"m": [1, 3], "h": [5000000000, 15000000000]}, None, {"m": [2, 3], "a": [0, 0]}]


def counts_for(totals, cols):
    n_mod = np.zeros((len(totals), len(cols)), dtype=np.uint64)
    n_valid = np.zeros_like(n_mod)
    for r, t in enumerate(totals):
        for k, c in enumerate(cols):
            if t and c in t:
                n_mod[r, k], n_valid[r, k] = t[c]
    return {"codes": [modkit_amd.code_repr(c) for c in cols], "n_mod": n_mod, "n_valid": n_valid, "contig_has_rows": [t is not None for t in totals]}


@pytest.mark.parametrize("cols,header", [
    (["a", "h", "m", "21839"], True),        # `a` is a forced column whose n_valid is 0 everywhere; the ChEBI code sorts after the letters
    (["a", "h", "m", "21839"], False),       # --no-header
    (["m"], True),
    ([], True),                              # no columns at all
    ([], False),
], ids=["all", "no_header", "m_only", "no_columns", "no_columns_no_header"])
def test_table_writer_equals_the_model(tmp_path, cols, header):
    regions = model.parse_regions(TABLE_BED)
    assert sorted(cols, key=model.code_key) == cols
    want = model.format_table(regions, TABLE_TOTALS, cols, header)
    rs = modkit_amd.RegionSet(write(tmp_path, TABLE_BED), ["chr1", "chr2"])
    out = str(tmp_path / "t.tsv")
    rs.write_table(counts_for(TABLE_TOTALS, cols), out, header=header)
    assert open(out).read() == want
    rs.close()


def test_table_pins():
    """percent 0, 100, 1/3, 2/3 and an empty total through f32 Display; the dropped region; the absent columns"""
    regions = model.parse_regions(TABLE_BED)
    text = model.format_table(regions, TABLE_TOTALS, ["a", "h", "m", "21839"], True)
    lines = text.split("\n")
    assert lines[0].split("\t") == ["chrom", "start", "end", "name", "strand", "count_a", "count_valid_a", "percent_a", "count_h", "count_valid_h",
                                    "percent_h", "count_m", "count_valid_m", "percent_m", "count_21839", "count_valid_21839", "percent_21839"]
    assert lines[1] == "chr1\t0\t10\tzero\t+\t0\t0\t0\t0\t0\t0\t0\t7\t0\t3\t3\t100"
    assert lines[2] == "chr1\t0\t10\tfull\t-\t0\t0\t0\t0\t0\t0\t9\t9\t100\t0\t0\t0"
    # (15 000 000 000 is no f32: `as f32` rounds it to 15 000 000 512, so this third comes out one step lower than 1 / 3 does)
    assert lines[3] == "chr2\t5\t50\tthird\t.\t0\t0\t0\t5000000000\t15000000000\t33.333332\t1\t3\t33.333336\t0\t0\t0"
    assert lines[4] == "chr2\t7\t7\ttwo thirds\t.\t0\t0\t0\t0\t0\t0\t2\t3\t66.66667\t0\t0\t0"
    assert lines[5:] == [""]   # `gone` is dropped
    assert model.rust_f32(np.float32(1) / np.float32(3) * np.float32(100)) == "33.333336"


# ---- the model on the reference's data, totals added up by hand from the golden lines
GOLDEN_BED = ("oligo_1512_adapters\t9\t41\tearly\t0\t.\n"        # positions 9, 19, 40
              "oligo_1512_adapters\t19\t20\tnested\t.\t.\n"      # position 19 alone, inside `early`
              "oligo_1512_adapters\t69\t74\tmixed\t0.5\t.\n"     # 69 +, 70 -, 72 +, 73 -
              "chr_not_there\t0\t100\tabsent\t0\t.\n"
              "oligo_1512_adapters\t63\t66\tminus\t0\t-\n")      # the '-' rows of 63, 64, 65 (63 also has '+' rows: not counted)


def test_model_on_the_golden_bedmethyl():
    text = open(GOLDEN).read()
    rows = [l.split("\t") for l in text.splitlines()]
    def line(pos, code, strand):   # (valid coverage, modified) of one golden line, checked to be there exactly once
        hit = [r for r in rows if r[1] == str(pos) and r[3] == code and r[5] == strand]
        assert len(hit) == 1
        return int(hit[0][9]), int(hit[0][11])
    # the lines themselves, as read off the golden file
    assert [line(9, "h", "+"), line(19, "h", "+"), line(40, "h", "-")] == [(4, 2), (6, 4), (1, 1)]
    assert [line(9, "m", "+"), line(19, "m", "+"), line(40, "m", "-")] == [(4, 1), (6, 0), (1, 0)]
    assert [line(63, "h", "-"), line(64, "h", "-"), line(65, "h", "-")] == [(1, 1), (2, 1), (2, 0)]
    assert [line(63, "m", "-"), line(64, "m", "-"), line(65, "m", "-")] == [(1, 0), (2, 1), (2, 2)]
    assert [line(69, "h", "+"), line(70, "h", "-"), line(72, "h", "+"), line(73, "h", "-")] == [(5, 0), (4, 0), (6, 2), (4, 0)]
    assert [line(69, "m", "+"), line(70, "m", "-"), line(72, "m", "+"), line(73, "m", "-")] == [(5, 5), (4, 4), (6, 4), (4, 4)]
    assert line(63, "h", "+") == (6, 1)   # the '+' row the stranded region must leave out
    # ... added up by hand: (n_mod, n_valid) of h then m
    by_hand = {"early": ((7, 11), (1, 11)), "nested": ((4, 6), (0, 6)), "mixed": ((2, 19), (17, 19)), "minus": ((2, 5), (3, 5))}
    got = model.stats_table(text, GOLDEN_BED)
    lines = got.splitlines()
    assert lines[0] == "chrom\tstart\tend\tname\tstrand\tcount_h\tcount_valid_h\tpercent_h\tcount_m\tcount_valid_m\tpercent_m"
    assert [l.split("\t")[3] for l in lines[1:]] == ["early", "nested", "mixed", "minus"]   # `absent` is dropped, file order otherwise
    for l in lines[1:]:
        f = l.split("\t")
        (hm, hv), (mm, mv) = by_hand[f[3]]
        assert [int(f[5]), int(f[6]), int(f[8]), int(f[9])] == [hm, hv, mm, mv], f[3]
        assert f[7] == model.rust_f32(np.float32(hm) / np.float32(hv) * np.float32(100)) and f[10] == model.rust_f32(np.float32(mm) / np.float32(mv) * np.float32(100))
    assert lines[1].split("\t")[7] == "63.636364" and lines[2].split("\t")[10] == "0" and lines[4].split("\t")[4] == "-"
    # a code filter, a coverage floor and --no-header on the same data
    only_m = model.stats_table(text, GOLDEN_BED, codes=["m"], min_coverage=5, header=False).splitlines()
    assert only_m[0].split("\t")[5:7] == ["0", "6"]      # early: position 19 alone has coverage >= 5
    assert only_m[3].split("\t")[5:] == ["0", "0", "0"]  # minus: no row reaches 5
