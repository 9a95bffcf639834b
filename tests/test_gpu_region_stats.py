"""Region statistics on the device (`modkit stats` over rows in HBM: mkp_stats.hip behind mkp_stats_begin / _add_rows / _add_resident / _get
and `modkit pileup --region-stats`) against the independent model of tests/region_stats_model.py.
1. directed rows through stats_add_rows: wave tails, the 4096-row chunk edge, several chunks per region, a thousand regions of every kind;
2. fused runs: a pileup that writes its bedMethyl AND the table — the model, fed that bedMethyl file, must give the table byte for byte;
3. --region-stats-only; 4. the file form modkit_amd.stats; 5. the refusals."""
import os

import numpy as np
import pytest

import modkit_amd
import region_stats_model as model
from pileup_cases import FIX, REF

pytestmark = pytest.mark.gpu

BC = os.path.join(FIX, "bc_anchored_10_reads.sorted.bam")
HG = os.path.join(FIX, "HG002_small.ch20._other.sorted.bam")
BED3 = os.path.join(FIX, "CGI_ladder_3.6kb_ref_CG_bed3.bed")                 # the reference's own region files (tests/resources), as data
BED6 = os.path.join(FIX, "CGI_ladder_3.6kb_ref_include_positions.bed")
U32 = (1 << 32) - 1
CODES16 = ["m", "h", "a", "c", "f", "g", "e", "b", "o", "n", "17802", "21839", "76792", "19228", "17596", "16964"]


# ---- 1. directed rows
def make_rows(n, seed, codes=("m", "h", "21839")):
    """n bedMethyl rows of one contig, ascending positions with repeats (a position has a row per strand and code), every strand letter,
    coverage 0 .. 20 with some at 2^32 - 1 so that totals pass 2^32"""
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.integers(0, 4, size=n)).astype(np.uint32) + 7 if n else np.zeros(0, dtype=np.uint32)
    strand = np.frombuffer(b"+-.", dtype=np.uint8)[rng.integers(0, 3, size=n)]
    code = np.array([modkit_amd.code_repr(codes[k]) for k in rng.integers(0, len(codes), size=n)], dtype=np.uint32)
    n_valid = rng.integers(0, 21, size=n).astype(np.uint32)
    n_valid[rng.random(n) < 0.05] = U32
    n_mod = (n_valid * rng.random(n)).astype(np.uint32)
    return {"pos": pos, "strand": strand, "code_repr": code, "n_valid": n_valid, "n_mod": n_mod}


def code_text(c):
    c = int(c)
    return str(c & 0x7fffffff) if c & 0x80000000 else chr(c)


def records_of(rows, chrom="c0"):
    return [(chrom, int(p), code_text(c), chr(s), int(v), int(m)) for p, s, c, v, m in
            zip(rows["pos"], rows["strand"], rows["code_repr"], rows["n_valid"], rows["n_mod"])]


def make_regions(rows, n_regions, seed, chrom="c0"):
    """(chrom, start, end, name, strand) in drawn (unsorted) order: empty, single positions, nested and identical ones, the whole contig,
    beyond the last row, ending exactly on a row and one past it — with every strand rule"""
    rng = np.random.default_rng(seed)
    pos = rows["pos"]
    last = int(pos[-1]) if len(pos) else 50
    at_row = (lambda: int(pos[rng.integers(0, len(pos))])) if len(pos) else (lambda: int(rng.integers(0, 50)))
    out = []
    while len(out) < n_regions:
        kind = int(rng.integers(0, 9))
        if kind == 0:
            s = at_row(); r = (s, s)                                  # empty
        elif kind == 1:
            s = at_row(); r = (s, s + 1)                              # one position
        elif kind == 2 and out:
            o = out[int(rng.integers(0, len(out)))]; r = (o[1], o[2])   # identical to an earlier one
        elif kind == 3 and out:
            o = out[int(rng.integers(0, len(out)))]; mid = (o[1] + o[2]) // 2; r = (o[1] + (mid - o[1]) // 2, mid)   # nested in an earlier one
        elif kind == 4:
            r = (0, last + 10)                                        # the whole contig
        elif kind == 5:
            r = (last + 1 + int(rng.integers(0, 5)), last + 100)      # beyond the last row
        elif kind == 6:
            e = at_row(); r = (max(0, e - int(rng.integers(1, 200))), e)       # ends exactly on a row (which is then outside)
        elif kind == 7:
            e = at_row(); r = (max(0, e - int(rng.integers(1, 200))), e + 1)   # ... and one past it (inside)
        else:
            a, b = sorted((int(rng.integers(0, last + 20)), int(rng.integers(0, last + 20)))); r = (a, b)
        out.append((chrom, r[0], r[1], None, "+-."[int(rng.integers(0, 3))]))
    return out


def fast_totals(rows, regions, codes, min_coverage):
    """the same totals with numpy (checked against the model below wherever the model's double loop is affordable)"""
    keep = rows["n_valid"].astype(np.uint64) >= min_coverage
    if codes is not None:
        keep &= np.isin(rows["code_repr"], [modkit_amd.code_repr(c) for c in codes])
    out = []
    for _c, s, e, _n, strand in regions:
        lo, hi = np.searchsorted(rows["pos"], [s, e], side="left") if e > s else (0, 0)
        sl = slice(lo, hi)
        k = keep[sl] & ((rows["strand"][sl] == ord(".")) | (strand == ".") | (rows["strand"][sl] == ord(strand)))
        agg = {}
        for c in np.unique(rows["code_repr"][sl][k]):
            m = k & (rows["code_repr"][sl] == c)
            agg[code_text(c)] = [int(rows["n_mod"][sl][m].astype(np.uint64).sum()), int(rows["n_valid"][sl][m].astype(np.uint64).sum())]
        out.append(agg)
    return out


def device_totals(pieces, regions, codes=None, min_coverage=1, tids={"c0": 0}):
    """pieces = [(tid, rows), ...] added in order; returns the stats_get dict"""
    ctx = modkit_amd.Context()
    try:
        ctx.stats_begin([(tids.get(c, -1), s, e, st) for c, s, e, _n, st in regions], codes=codes, min_coverage=min_coverage)
        for tid, rows in pieces:
            ctx.stats_add_rows(tid, rows)
        return ctx.stats_get()
    finally:
        ctx.close()


def assert_same(dev, totals, codes):
    cols = model.columns(totals, codes)
    assert [code_text(c) for c in dev["codes"]] == cols
    assert list(dev["contig_has_rows"]) == [0 if t is None else 1 for t in totals]
    want_mod = np.array([[(t or {}).get(c, (0, 0))[0] for c in cols] for t in totals], dtype=np.uint64).reshape(len(totals), len(cols))
    want_valid = np.array([[(t or {}).get(c, (0, 0))[1] for c in cols] for t in totals], dtype=np.uint64).reshape(len(totals), len(cols))
    assert np.array_equal(dev["n_mod"], want_mod) and np.array_equal(dev["n_valid"], want_valid)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 20001])
def test_directed_rows_one_call(n):
    rows = make_rows(n, seed=100 + n)
    regions = make_regions(rows, 1000, seed=200 + n)
    dev = device_totals([(0, rows)], regions)
    if n <= 4097:
        totals = model.region_totals(records_of(rows), regions) if n else [None] * len(regions)   # (no row at all: the contig is not listed)
    else:   # the model's double loop on a sample of the regions pins the numpy form, which then checks them all
        totals = fast_totals(rows, regions, None, 1)
        sample = list(range(0, len(regions), 10))
        assert [totals[i] for i in sample] == model.region_totals(records_of(rows), [regions[i] for i in sample])
        assert any(s == 0 and e > int(rows["pos"][-1]) for _c, s, e, _n, _st in regions)   # the whole contig: five chunks for one region
    assert_same(dev, totals, None)
    if n >= 4095:
        assert int(dev["n_valid"].max()) > U32   # totals pass 2^32


@pytest.mark.parametrize("min_coverage", [0, 1, 5])
@pytest.mark.parametrize("codes", [None, ["h", "21839", "x"]], ids=["all_codes", "code_filter"])
def test_directed_rows_options(min_coverage, codes):
    rows = make_rows(700, seed=11)
    regions = make_regions(rows, 1000, seed=12)
    dev = device_totals([(0, rows)], regions, codes=codes, min_coverage=min_coverage)
    totals = model.region_totals(records_of(rows), regions, codes, min_coverage)
    assert totals == fast_totals(rows, regions, codes, min_coverage)
    assert_same(dev, totals, codes)
    if codes is None and min_coverage == 0:
        assert any(v == [0, 0] for t in totals for v in t.values())   # a counted row without coverage still makes the column entry


def test_sixteen_codes_run_seventeen_are_refused():
    rows = make_rows(900, seed=21, codes=CODES16)
    regions = make_regions(rows, 200, seed=22)
    totals = model.region_totals(records_of(rows), regions)
    dev = device_totals([(0, rows)], regions)
    assert len(dev["codes"]) == 16
    assert_same(dev, totals, None)
    rows17 = make_rows(900, seed=21, codes=CODES16 + ["z"])
    with pytest.raises(modkit_amd.MkpError) as e:
        device_totals([(0, rows17)], regions)
    assert e.value.status == -3   # MKP_E_UNSUPPORTED
    # a seventeenth code OUTSIDE every region claims nothing
    outside = [("c0", int(rows17["pos"][-1]) + 5, int(rows17["pos"][-1]) + 9, None, ".")]
    assert len(device_totals([(0, rows17)], outside)["codes"]) == 0


def test_rows_cut_into_three_calls_give_the_same_table():
    rows = make_rows(9000, seed=31)
    regions = make_regions(rows, 1000, seed=32)
    one = device_totals([(0, rows)], regions)
    cut = lambda a, b: {k: v[a:b] for k, v in rows.items()}
    three = device_totals([(0, cut(0, 2999)), (0, cut(2999, 7301)), (0, cut(7301, 9000))], regions)
    for k in one:
        assert np.array_equal(one[k], three[k]), k
    assert_same(one, fast_totals(rows, regions, None, 1), None)


def test_two_contigs_one_without_rows():
    rows = make_rows(500, seed=41)
    regions = make_regions(rows, 60, seed=42, chrom="c0") + make_regions(rows, 40, seed=43, chrom="c1") + [("elsewhere", 0, 100, None, ".")]
    order = np.random.default_rng(44).permutation(len(regions))
    regions = [regions[i] for i in order]
    dev = device_totals([(0, rows)], regions, tids={"c0": 0, "c1": 1})
    totals = model.region_totals(records_of(rows), regions)
    assert sum(t is None for t in totals) == 41
    assert_same(dev, totals, None)


def test_misuse():
    ctx = modkit_amd.Context()
    try:
        rows = make_rows(10, seed=51)
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.stats_add_rows(0, rows)   # before stats_begin
        assert e.value.status == -1
        ctx.stats_begin([(0, 0, 100, ".")])
        down = {k: v[::-1].copy() for k, v in rows.items()}
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.stats_add_rows(0, down)
        assert e.value.status == -1 and "ascending" in str(e.value)
        ctx.set_partition_tags(["HP"])
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.stats_add_resident()
        assert e.value.status == -1 and "partition" in str(e.value)
        ctx.set_partition_tags([])
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.stats_begin([(0, 9, 3, ".")])   # start > end
        assert e.value.status == -1
    finally:
        ctx.close()


# ---- 2. fused runs
STRANDED_BC = ("oligo_1512_adapters\t0\t60\thead\t0\t+\noligo_1512_adapters\t0\t60\thead\t0\t-\noligo_1512_adapters\t0\t5000\tall\t.\t.\n"
               "oligo_741_adapters\t20\t70\twindow\t1.5\t-\noligo_741_adapters\t30\t30\tempty\t0\t+\nno_such_contig\t0\t10\tnowhere\t0\t.\n"
               "oligo_1512_adapters\t63\t66\tminus\t0\t-\n")
# HG002 rows lie on chr20:60000-170000; the run below cuts the window at 90000, 120000 and 150000
STRANDED_HG = ("chr20\t0\t1000000\twhole\t0\t.\nchr20\t65000\t125000\tstraddles two seams\t0\t.\nchr20\t89990\t90010\tacross one seam\t0\t+\n"
               "chr20\t119000\t121000\tacross\t0\t-\nchr20\t70000\t70200\tsmall\t0\t.\nchr20\t90000\t90000\tempty at a seam\t0\t.\n"
               "chr1\t0\t100000\tno rows here\t0\t.\nchr20\t120000\t150000\texactly one shard\t0\t.\n")
HG_FLAGS = ["--no-filtering", "--force-allow-implicit", "--region", "chr20:60000-170000", "--shard-bp", "30000", "-i", "10000"]
FUSED = {
    "nofilt": (BC, ["-i", "25", "--no-filtering", "--only-tabs"]),                                       # event pipeline, no slots
    "nofilt_host_ingest": (BC, ["-i", "25", "--no-filtering", "--only-tabs", "--host-ingest"]),
    "cpg_combine_strands": (BC, ["--no-filtering", "--cpg", "--ref", REF, "--combine-strands"]),         # slot pipeline, '.' rows
    "two_motifs": (BC, ["--no-filtering", "--motif", "CG", "0", "--motif", "CGCG", "2", "--ref", REF]),  # a row per motif id, all counted
    "hg002_shards": (HG, HG_FLAGS),
    "hg002_shards_host_ingest": (HG, HG_FLAGS + ["--host-ingest"]),
}


def region_beds(tmp_path, case):
    if case.startswith("hg002"):
        p = tmp_path / "hg.bed"; p.write_text(STRANDED_HG)
        return {"stranded": str(p)}
    p = tmp_path / "bc.bed"; p.write_text(STRANDED_BC)
    return {"bed3": BED3, "bed6": BED6, "stranded": str(p)}


def fused(tmp_path, case, bed, extra=(), tag="f"):
    bam, flags = FUSED[case]
    out, table = str(tmp_path / (tag + ".bed")), str(tmp_path / (tag + ".tsv"))
    ctx = modkit_amd.Context()
    try:
        rep = ctx.pileup_run([bam, out] + flags + ["--region-stats", bed, "--region-stats-out", table] + list(extra))
    finally:
        ctx.close()
    return out, table, rep


@pytest.mark.parametrize("case", sorted(FUSED))
def test_fused_table_is_the_model_on_the_runs_own_bedmethyl(tmp_path, case):
    for name, bed in region_beds(tmp_path, case).items():
        out, table, rep = fused(tmp_path, case, bed, tag=name)
        text = open(out).read()
        assert len(text.splitlines()) == rep.n_rows > 0
        want = model.stats_table(text, open(bed).read())
        assert open(table).read() == want, name
        assert len(want.splitlines()) > 2
        if case.startswith("nofilt"):   # the chain reaches the reference: this run's bedMethyl is its golden file
            assert text == open(os.path.join(FIX, "modbam.modpileup_nofilt.methyl.bed")).read()
        if case.startswith("hg002"):
            assert rep.n_shards > 1
            head, whole = (l.split("\t") for l in want.splitlines()[:2])
            first_code = head[5][len("count_"):]
            assert whole[3] == "whole" and int(whole[6]) == sum(int(l.split()[9]) for l in text.splitlines() if l.split()[3].split(",")[0] == first_code)
        if case == "two_motifs":
            assert any("," in l.split()[3] for l in text.splitlines())
        if case == "cpg_combine_strands":
            assert {l.split()[5] for l in text.splitlines()} == {"."}


def test_fused_options(tmp_path):
    bed = region_beds(tmp_path, "nofilt")["stranded"]
    out, table, _ = fused(tmp_path, "nofilt", bed, ["--region-stats-codes", "m,21839", "--region-stats-min-coverage", "5", "--region-stats-no-header"])
    want = model.stats_table(open(out).read(), open(bed).read(), codes=["m", "21839"], min_coverage=5, header=False)
    assert open(table).read() == want and want


# ---- 3. --region-stats-only, 4. the file form
@pytest.mark.parametrize("case", ["nofilt", "cpg_combine_strands", "hg002_shards"])
def test_stats_only_and_file_form(tmp_path, case):
    bed = region_beds(tmp_path, case)["stranded"]
    out, table, rep = fused(tmp_path, case, bed)
    out2, table2, rep2 = fused(tmp_path, case, bed, ["--region-stats-only"], tag="only")
    assert open(table2).read() == open(table).read()
    assert not os.path.exists(out2)
    assert rep2.n_rows == rep.n_rows > 0 and rep2.n_shards == rep.n_shards
    table3 = str(tmp_path / "file_form.tsv")
    modkit_amd.stats(out, bed, table3)
    assert open(table3).read() == open(table).read()


def test_file_form_takes_multi_motif_names(tmp_path):
    bed = region_beds(tmp_path, "two_motifs")["bed6"]
    out, table, _ = fused(tmp_path, "two_motifs", bed)
    table3 = str(tmp_path / "file_form.tsv")
    modkit_amd.stats(out, bed, table3, codes=["h"], min_coverage=2, header=False)
    assert open(table3).read() == model.stats_table(open(out).read(), open(bed).read(), codes=["h"], min_coverage=2, header=False)


# ---- 5. refusals
def test_refusals(tmp_path):
    bed = region_beds(tmp_path, "nofilt")["stranded"]
    stats = ["--region-stats", bed, "--region-stats-out", str(tmp_path / "t.tsv")]
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.pileup_hemi([os.path.join(FIX, "duplex_modcalls_sort.bam"), "-o", str(tmp_path / "h.bed"), "--cpg", "--ref", REF] + stats)
    assert e.value.status == -1 and "unexpected argument '--region-stats'" in str(e.value)
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.pileup([BC, str(tmp_path / "parts"), "--no-filtering", "--partition-tag", "HP"] + stats)
    assert e.value.status == -1 and "--partition-tag" in str(e.value)
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.pileup([BC, str(tmp_path / "w.bed"), "--no-filtering", "--gpus-world", "2", "--gpus-rank", "0"] + stats)
    assert e.value.status == -3
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.pileup([BC, str(tmp_path / "x.bed"), "--no-filtering", "--region-stats-only"])
    assert e.value.status == -1
    assert not os.path.exists(str(tmp_path / "t.tsv"))
