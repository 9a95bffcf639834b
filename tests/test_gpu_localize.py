"""Localize on the device (`modkit localize` over rows in HBM: mkp_localize.hip behind mkp_localize_begin / _add_rows / _add_resident / _get
and `modkit pileup --localize`) against the independent model of tests/localize_model.py.
1. directed rows through localize_add_rows: wave tails, tables that end before, on and after a tile edge, a thousand regions of every kind;
2. the options, the code-slot paths, seams, contigs, misuse;
3. fused runs: a pileup that writes its bedMethyl AND the table — the model, fed that bedMethyl file, must give the table byte for byte;
4. --localize-only, --localize with --region-stats, the file form modkit_amd.localize; 5. the refusals."""
import gzip
import os
import struct

import numpy as np
import pytest

import modkit_amd
import localize_model as model
from pileup_cases import FIX, REF

pytestmark = pytest.mark.gpu

BC = os.path.join(FIX, "bc_anchored_10_reads.sorted.bam")
HG = os.path.join(FIX, "HG002_small.ch20._other.sorted.bam")
BED3 = os.path.join(FIX, "CGI_ladder_3.6kb_ref_CG_bed3.bed")                 # the reference's own region files (tests/resources), as data
BED6 = os.path.join(FIX, "CGI_ladder_3.6kb_ref_include_positions.bed")
U32 = (1 << 32) - 1
TO = modkit_amd.localize_tile_offsets()
CODES16 = ["m", "h", "a", "c", "f", "g", "e", "b", "o", "n", "17802", "21839", "76792", "19228", "17596", "16964"]
INVALID, UNSUPPORTED = -1, -3


# ---- 1. directed rows
def make_rows(n, seed, codes=("m", "h", "21839")):
    """n bedMethyl rows of one contig, ascending positions with repeats (a position has a row per strand and code), every strand letter,
    coverage 0 .. 20 with some at 2^32 - 1 so that totals pass 2^32 through the carry path"""
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


def contig_length(rows):
    return (int(rows["pos"][-1]) if len(rows["pos"]) else 50) + 3


def make_regions(rows, n_regions, seed, window, chrom="c0"):
    """(chrom, start, end, strand) in drawn (unsorted) order: 200 regions on one anchor, then windows clipped at 0, clipped at the contig
    end, behind the contig end, identical repeats, start > end and windows anywhere — with every strand"""
    rng = np.random.default_rng(seed)
    pos, length = rows["pos"], contig_length(rows)
    at_row = (lambda: int(pos[rng.integers(0, len(pos))])) if len(pos) else (lambda: int(rng.integers(0, 50)))
    strand = lambda: "+-."[int(rng.integers(0, 3))]
    one = at_row()
    out = [(chrom, one, one + 2, strand()) for _ in range(200)]
    while len(out) < n_regions:
        kind = int(rng.integers(0, 7))
        if kind == 0:
            s = int(rng.integers(0, window + 2)); r = (s, s + int(rng.integers(0, 3)))                 # clipped at 0 (or just not)
        elif kind == 1:
            s = max(0, length - int(rng.integers(0, window + 3))); r = (s, s + int(rng.integers(0, 5)))   # clipped at the contig end
        elif kind == 2:
            s = length + window + 1 + int(rng.integers(0, 50)); r = (s, s + 10)                         # behind it: an empty window
        elif kind == 3:
            o = out[int(rng.integers(0, len(out)))]; r = (o[1], o[2])                                   # identical to an earlier one
        elif kind == 4:
            s = at_row() + int(rng.integers(1, 50)); r = (s, max(0, s - int(rng.integers(1, 40))))      # start > end
        else:
            s = max(0, at_row() - int(rng.integers(0, 9))); r = (s, s + int(rng.integers(0, 30)))
        out.append((chrom, r[0], r[1], strand()))
    return [out[i] for i in rng.permutation(len(out))]


def fast_counts(rows, regions, length, window, stranded=None, stranded_features=None):
    """the model's totals with numpy ({code: {offset: [n_mod, n_valid]}}; pinned by the model wherever both are run)"""
    pos, strand = rows["pos"].astype(np.int64), rows["strand"]
    ucodes = np.unique(rows["code_repr"])
    slot = np.searchsorted(ucodes, rows["code_repr"])
    n_off = 2 * window + 1
    acc = np.zeros((3, len(ucodes), n_off), dtype=np.uint64)
    for _c, start, end, rs in regions:
        ws, we, anchor = model.window_of(start, end, window, length)
        if we <= ws:
            continue
        lo, hi = np.searchsorted(pos, [ws, we], side="left")
        sl = slice(lo, hi)
        fetch = stranded_features if stranded_features is not None else rs
        keep = (strand[sl] == ord(".")) | (fetch == ".") | (strand[sl] == ord(fetch))
        if stranded is not None:
            ov = (strand[sl] == ord(".")) | (rs == ".") | (strand[sl] == ord(rs))
            keep &= ov if stranded == "same" else ~ov
        idx = (slot[sl][keep], (anchor - pos[sl][keep]) + window)
        np.add.at(acc[0], idx, rows["n_mod"][sl][keep].astype(np.uint64))
        np.add.at(acc[1], idx, rows["n_valid"][sl][keep].astype(np.uint64))
        np.add.at(acc[2], idx, np.uint64(1))
    return {code_text(c): {int(o) - window: [int(acc[0, k, o]), int(acc[1, k, o])] for o in np.nonzero(acc[2, k])[0]}
            for k, c in enumerate(ucodes) if acc[2, k].any()}


def device_counts(pieces, regions, lengths, window, stranded=None, stranded_features=None, tids={"c0": 0}):
    """pieces = [(tid, rows), ...] added in order; returns the localize_get dict"""
    ctx = modkit_amd.Context()
    try:
        ctx.localize_begin([(tids.get(c, -1), s, e, st) for c, s, e, st in regions], lengths, window=window, stranded=stranded,
                           stranded_features=stranded_features)
        for tid, rows in pieces:
            ctx.localize_add_rows(tid, rows)
        return ctx.localize_get()
    finally:
        ctx.close()


def cells_of(dev):
    """the localize_get dict as the model's {code: {offset: [n_mod, n_valid]}}"""
    w = dev["window"]
    assert dev["n_mod"].shape == dev["n_valid"].shape == dev["n_rows"].shape == (len(dev["codes"]), 2 * w + 1)
    assert list(dev["codes"]) == sorted(dev["codes"]) and all(r.any() for r in dev["n_rows"])
    assert not dev["n_mod"][dev["n_rows"] == 0].any() and not dev["n_valid"][dev["n_rows"] == 0].any()
    return {code_text(c): {int(o) - w: [int(dev["n_mod"][k, o]), int(dev["n_valid"][k, o])] for o in np.nonzero(dev["n_rows"][k])[0]}
            for k, c in enumerate(dev["codes"])}


@pytest.mark.parametrize("window", [0, 1, 7, TO // 2 - 1, TO // 2, TO // 2 + 1, 2000])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 20001])
def test_directed_rows_one_call(n, window):
    rows = make_rows(n, seed=100 + n)
    length = contig_length(rows)
    regions = make_regions(rows, 1000, seed=200 + n, window=window)
    assert sum(s > e for _c, s, e, _st in regions) > 20 and {st for *_r, st in regions} == {"+", "-", "."}
    assert sum(model.window_of(s, e, window, length)[1] <= model.window_of(s, e, window, length)[0] for _c, s, e, _st in regions) > 20
    if n == 0:   # no row at all: the contig is not listed, no region is left, the reference fails
        with pytest.raises(model.LocalizeError):
            model.offset_totals([], regions, {"c0": length}, window)
        with pytest.raises(modkit_amd.MkpError) as e:
            device_counts([(0, rows)], regions, [length], window)
        assert e.value.status == INVALID
        return
    dev = device_counts([(0, rows)], regions, [length], window)
    want = fast_counts(rows, regions, length, window)
    if n <= 257:
        assert want == model.offset_totals(records_of(rows), regions, {"c0": length}, window)
    else:   # the model's double loop on every tenth region pins the numpy form, which then checks them all
        sample = regions[::10]
        assert fast_counts(rows, sample, length, window) == model.offset_totals(records_of(rows), sample, {"c0": length}, window)
    assert cells_of(dev) == want
    if n >= 255:
        assert int(dev["n_valid"].max()) > U32   # totals pass 2^32
    if n == 20001:   # (a contig shorter than the window clips every window, and the offsets stay away from the table's ends)
        assert min(min(t) for t in want.values()) == -window and max(max(t) for t in want.values()) == window   # used up to both ends


@pytest.mark.parametrize("stranded_features", [None, "+", "-", "."])
@pytest.mark.parametrize("stranded", [None, "same", "opposite"])
def test_directed_rows_options(stranded, stranded_features):
    rows = make_rows(700, seed=11)
    length = contig_length(rows)
    regions = make_regions(rows, 1000, seed=12, window=7)
    dev = device_counts([(0, rows)], regions, [length], 7, stranded, stranded_features)
    want = model.offset_totals(records_of(rows), regions, {"c0": length}, 7, stranded, stranded_features)
    assert want == fast_counts(rows, regions, length, 7, stranded, stranded_features)
    assert cells_of(dev) == want
    assert want or stranded == "opposite"


def test_a_row_without_coverage_makes_its_cell():
    rows = {"pos": np.array([40, 40, 47], dtype=np.uint32), "strand": np.frombuffer(b"+-+", dtype=np.uint8),
            "code_repr": np.array([ord("m"), ord("h"), ord("m")], dtype=np.uint32), "n_valid": np.array([0, 3, 0], dtype=np.uint32),
            "n_mod": np.array([0, 1, 0], dtype=np.uint32)}
    regions = [("c0", 40, 43, ".")]   # mp 41, window [38, 43), anchor 40: position 47 is outside
    dev = device_counts([(0, rows)], regions, [100], 2)
    assert cells_of(dev) == {"m": {0: [0, 0]}, "h": {0: [1, 3]}} == model.offset_totals(records_of(rows), regions, {"c0": 100}, 2)
    assert dev["n_rows"].tolist() == [[0, 0, 1, 0, 0], [0, 0, 1, 0, 0]]


def test_five_codes_take_the_slot_path_beyond_lds():
    rows = make_rows(3000, seed=15, codes=CODES16[:5])
    length = contig_length(rows)
    window = TO // 2 + 1
    regions = make_regions(rows, 1000, seed=16, window=window)
    dev = device_counts([(0, rows)], regions, [length], window)
    assert len(dev["codes"]) == 5
    assert cells_of(dev) == fast_counts(rows, regions, length, window)
    assert all(int(r.max()) > U32 for r in dev["n_valid"])   # every code, the per-row one too, carries past 2^32


def test_sixteen_codes_run_seventeen_are_refused():
    rows = make_rows(900, seed=21, codes=CODES16)
    length = contig_length(rows)
    regions = make_regions(rows, 300, seed=22, window=9)
    dev = device_counts([(0, rows)], regions, [length], 9)
    assert len(dev["codes"]) == 16
    assert cells_of(dev) == model.offset_totals(records_of(rows), regions, {"c0": length}, 9)
    rows17 = make_rows(900, seed=21, codes=CODES16 + ["z"])
    with pytest.raises(modkit_amd.MkpError) as e:
        device_counts([(0, rows17)], regions, [length], 9)
    assert e.value.status == UNSUPPORTED
    # a seventeenth code OUTSIDE every window claims nothing: sixteen codes inside [0, 400), `z` beyond
    inside = make_rows(300, seed=23, codes=CODES16)
    far = make_rows(50, seed=24, codes=["z"])
    far["pos"] = far["pos"] + np.uint32(int(inside["pos"][-1]) + 500)
    both = {k: np.concatenate([inside[k], far[k]]) for k in inside}
    regions = [("c0", 100, 102, "."), ("c0", 200, 202, "+")]
    dev = device_counts([(0, both)], regions, [contig_length(both)], 60)
    assert cells_of(dev) == model.offset_totals(records_of(both), regions, {"c0": contig_length(both)}, 60)
    assert "z" not in cells_of(dev) and len(dev["codes"]) > 3


def test_rows_cut_into_three_calls_give_the_same_table():
    rows = make_rows(9000, seed=31)
    length = contig_length(rows)
    regions = make_regions(rows, 1000, seed=32, window=300)
    one = device_counts([(0, rows)], regions, [length], 300)
    cut = lambda a, b: {k: v[a:b] for k, v in rows.items()}
    three = device_counts([(0, cut(0, 2999)), (0, cut(2999, 7301)), (0, cut(7301, 9000))], regions, [length], 300)
    for k in one:
        assert np.array_equal(one[k], three[k]), k
    assert cells_of(one) == fast_counts(rows, regions, length, 300)


def test_two_contigs_one_without_rows_and_an_unlisted_one():
    rows = make_rows(500, seed=41)
    length = contig_length(rows)
    on_c0 = make_regions(rows, 260, seed=42, window=5)
    regions = on_c0 + make_regions(rows, 240, seed=43, window=5, chrom="c1") + [("elsewhere", 0, 100, "."), ("unsized", 20, 30, ".")]
    regions = [regions[i] for i in np.random.default_rng(44).permutation(len(regions))]
    # `unsized` has a tid beyond the sizes table, `elsewhere` none at all; c1 is sized and gets no row
    tids = {"c0": 0, "c1": 1, "unsized": 2}
    dev = device_counts([(0, rows)], regions, [length, length], 5, tids=tids)
    want = model.offset_totals(records_of(rows), regions, {"c0": length, "c1": length}, 5)
    assert want == model.offset_totals(records_of(rows), [r for r in regions if r[0] == "c0"], {"c0": length}, 5)
    assert cells_of(dev) == want
    # rows on the other contig only: c0's regions are dropped, c1's count
    dev = device_counts([(1, rows)], regions, [length, length], 5, tids=tids)
    assert cells_of(dev) == model.offset_totals(records_of(rows, "c1"), regions, {"c0": length, "c1": length}, 5)
    # no region on a sized contig: the begin fails; regions on a contig that no row came on: the get fails
    ctx = modkit_amd.Context()
    try:
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.localize_begin([(-1, 0, 100, "."), (2, 20, 30, ".")], [length, length], window=5)
        assert e.value.status == INVALID
        ctx.localize_begin([(1, 0, 100, ".")], [length, length], window=5)
        ctx.localize_add_rows(0, rows)
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.localize_get()
        assert e.value.status == INVALID
    finally:
        ctx.close()


def test_misuse():
    ctx = modkit_amd.Context()
    try:
        rows = make_rows(10, seed=51)
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.localize_add_rows(0, rows)   # before localize_begin
        assert e.value.status == INVALID
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.localize_add_resident()
        assert e.value.status == INVALID
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.localize_begin([(0, 0, 100, ".")], [1000], window=100001)   # over the cap
        assert e.value.status == UNSUPPORTED
        ctx.localize_begin([(0, 0, 100, ".")], [1000], window=100000)
        ctx.localize_begin([(0, 9, 3, ".")], [1000], window=5)   # start > end is no misuse here
        down = {k: v[::-1].copy() for k, v in rows.items()}
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.localize_add_rows(0, down)
        assert e.value.status == INVALID and "ascending" in str(e.value)
        ctx.set_partition_tags(["HP"])
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.localize_add_resident()
        assert e.value.status == INVALID and "partition" in str(e.value)
        ctx.set_partition_tags([])
        # a stats run and a localize run open on one context
        ctx.stats_begin([(0, 0, 100, ".")])
        ctx.stats_add_rows(0, rows)
        ctx.localize_add_rows(0, rows)
        assert int(ctx.stats_get()["n_valid"].sum()) > 0 and int(ctx.localize_get()["n_rows"].sum()) > 0
    finally:
        ctx.close()


# ---- 3. fused runs
STRANDED_BC = ("oligo_1512_adapters\t0\t60\thead\t0\t+\noligo_1512_adapters\t0\t60\thead\t0\t-\noligo_1512_adapters\t0\t5000\tall\t.\t.\n"
               "oligo_741_adapters\t20\t70\twindow\t1.5\t-\noligo_741_adapters\t30\t30\tempty\t0\t+\nno_such_contig\t0\t10\tnowhere\t0\t.\n"
               "oligo_1512_adapters\t63\t66\tminus\t0\t-\noligo_1512_adapters\t9\t3\tbackwards\t0\t.\nthis line fails\n")
# HG002 rows lie on chr20:60000-170000; the run below cuts the window at 90000, 120000 and 150000: with 2000 to either side the windows
# around 89990, 90000 and 150000 straddle one seam and the one of the long region two (its midpoint is 120005, the seam 120000 lies inside)
STRANDED_HG = ("chr20\t89990\t89990\tbefore a seam\t0\t.\nchr20\t90000\t90000\ton a seam\t0\t+\nchr20\t120005\t120005\tbehind a seam\t0\t-\n"
               "chr20\t150000\t150000\ton the last seam\t0\t.\nchr1\t0\t100000\tno rows here\t0\t.\nchr20\t118005\t122005\tsame anchor\t0\t.\n")
HG_FLAGS = ["--no-filtering", "--force-allow-implicit", "--region", "chr20:60000-170000", "--shard-bp", "30000", "-i", "10000"]
FUSED = {
    "nofilt": (BC, ["-i", "25", "--no-filtering", "--only-tabs"]),                                       # event pipeline, no slots
    "nofilt_host_ingest": (BC, ["-i", "25", "--no-filtering", "--only-tabs", "--host-ingest"]),
    "cpg_combine_strands": (BC, ["--no-filtering", "--cpg", "--ref", REF, "--combine-strands"]),         # slot pipeline, '.' rows
    "two_motifs": (BC, ["--no-filtering", "--motif", "CG", "0", "--motif", "CGCG", "2", "--ref", REF]),  # a row per motif id, all counted
    "hg002_shards": (HG, HG_FLAGS),
    "hg002_shards_host_ingest": (HG, HG_FLAGS + ["--host-ingest"]),
}


def bam_sizes(path):
    """`name<tab>length` per contig of a BAM header (SAM spec 4.2), as a genome-sizes text"""
    with gzip.open(path, "rb") as f:
        assert f.read(4) == b"BAM\x01"
        f.read(struct.unpack("<i", f.read(4))[0])
        out = []
        for _ in range(struct.unpack("<i", f.read(4))[0]):
            name = f.read(struct.unpack("<i", f.read(4))[0])[:-1].decode()
            out.append("%s\t%d\n" % (name, struct.unpack("<i", f.read(4))[0]))
    return "".join(out)


def region_beds(tmp_path, case):
    """{name: (bed path, window)}"""
    if case.startswith("hg002"):
        p = tmp_path / "hg.bed"; p.write_text(STRANDED_HG)
        return {"stranded": (str(p), 2000)}
    p = tmp_path / "bc.bed"; p.write_text(STRANDED_BC)
    return {"bed3": (BED3, 40), "bed6": (BED6, 3), "stranded": (str(p), 25)}


def fused(tmp_path, case, bed, window, extra=(), tag="f"):
    bam, flags = FUSED[case]
    out, table = str(tmp_path / (tag + ".bed")), str(tmp_path / (tag + ".tsv"))
    ctx = modkit_amd.Context()
    try:
        rep = ctx.pileup_run([bam, out] + flags + ["--localize", bed, "--localize-out", table, "--localize-window", str(window)] + list(extra))
    finally:
        ctx.close()
    return out, table, rep


@pytest.mark.parametrize("case", sorted(FUSED))
def test_fused_table_is_the_model_on_the_runs_own_bedmethyl(tmp_path, case):
    sizes = bam_sizes(FUSED[case][0])
    for name, (bed, window) in region_beds(tmp_path, case).items():
        out, table, rep = fused(tmp_path, case, bed, window, tag=name)
        text = open(out).read()
        assert len(text.splitlines()) == rep.n_rows > 0
        want = model.localize_table(text, open(bed).read(), sizes, window=window)
        assert open(table).read() == want, name
        assert len(want.splitlines()) > 2
        if case.startswith("nofilt"):   # the chain reaches the reference: this run's bedMethyl is its golden file
            assert text == open(os.path.join(FIX, "modbam.modpileup_nofilt.methyl.bed")).read()
        if case.startswith("hg002"):
            assert rep.n_shards > 1
        if case == "two_motifs":
            assert any("," in l.split()[3] for l in text.splitlines())
        if case == "cpg_combine_strands":
            assert {l.split()[5] for l in text.splitlines()} == {"."}


def test_fused_options(tmp_path):
    bed, _ = region_beds(tmp_path, "nofilt")["stranded"]
    sizes = bam_sizes(BC)
    out, table, _ = fused(tmp_path, "nofilt", bed, 30, ["--localize-stranded", "opposite", "--localize-stranded-features", "+"])
    want = model.localize_table(open(out).read(), open(bed).read(), sizes, window=30, stranded="opposite", stranded_features="+")
    assert open(table).read() == want and len(want.splitlines()) > 3
    out, table, _ = fused(tmp_path, "nofilt", bed, 30, ["--localize-stranded", "same"], tag="same")
    assert open(table).read() == model.localize_table(open(out).read(), open(bed).read(), sizes, window=30, stranded="same")
    # the default window is 2000
    bam, flags = FUSED["nofilt"]
    table = str(tmp_path / "default.tsv")
    modkit_amd.pileup([bam, str(tmp_path / "default.bed")] + flags + ["--localize", bed, "--localize-out", table])
    assert open(table).read() == model.localize_table(open(out).read(), open(bed).read(), sizes)


# ---- 4. --localize-only, --localize with --region-stats, the file form
STATS_BC = "oligo_1512_adapters\t0\t60\thead\t0\t+\noligo_1512_adapters\t0\t5000\tall\t.\t.\noligo_1512_adapters\t63\t66\tminus\t0\t-\n"
STATS_HG = "chr20\t0\t1000000\twhole\t0\t.\nchr20\t89990\t90010\tacross one seam\t0\t+\n"


@pytest.mark.parametrize("case", ["nofilt", "cpg_combine_strands", "hg002_shards"])
def test_localize_only_combined_and_file_form(tmp_path, case):
    bed, window = region_beds(tmp_path, case)["stranded"]
    out, table, rep = fused(tmp_path, case, bed, window)
    out2, table2, rep2 = fused(tmp_path, case, bed, window, ["--localize-only"], tag="only")
    assert open(table2).read() == open(table).read()
    assert not os.path.exists(out2)
    assert rep2.n_rows == rep.n_rows > 0 and rep2.n_shards == rep.n_shards
    # one run, both tables: each equals the one of its own run
    sbed = tmp_path / "stats.bed"; sbed.write_text(STATS_HG if case.startswith("hg002") else STATS_BC)
    stats_alone, stats_both = str(tmp_path / "stats_alone.tsv"), str(tmp_path / "stats_both.tsv")
    bam, flags = FUSED[case]
    modkit_amd.pileup([bam, str(tmp_path / "s.bed")] + flags + ["--region-stats", str(sbed), "--region-stats-out", stats_alone])
    out3, table3, rep3 = fused(tmp_path, case, bed, window, ["--region-stats", str(sbed), "--region-stats-out", stats_both], tag="both")
    assert open(table3).read() == open(table).read() and open(stats_both).read() == open(stats_alone).read()
    assert open(out3).read() == open(out).read() and len(open(stats_alone).read().splitlines()) > 2
    out4, table4, rep4 = fused(tmp_path, case, bed, window, ["--region-stats", str(sbed), "--region-stats-out", stats_both, "--region-stats-only"], tag="both_only")
    assert open(table4).read() == open(table).read() and open(stats_both).read() == open(stats_alone).read()
    assert not os.path.exists(out4) and rep4.n_rows == rep.n_rows
    # the file form on the run's bedMethyl
    sizes = tmp_path / "genome.sizes"; sizes.write_text(bam_sizes(bam))
    table5 = str(tmp_path / "file_form.tsv")
    modkit_amd.localize(out, bed, str(sizes), table5, window=window)
    assert open(table5).read() == open(table).read()


def test_file_form_options_and_multi_motif_names(tmp_path):
    bed, _ = region_beds(tmp_path, "two_motifs")["bed6"]
    out, table, _ = fused(tmp_path, "two_motifs", bed, 12)
    sizes = tmp_path / "genome.sizes"; sizes.write_text(bam_sizes(BC) + "extra\t5\n")
    table2 = str(tmp_path / "file_form.tsv")
    modkit_amd.localize(out, bed, str(sizes), table2, window=12, stranded="same", stranded_features="-")
    want = model.localize_table(open(out).read(), open(bed).read(), sizes.read_text(), window=12, stranded="same", stranded_features="-")
    assert open(table2).read() == want and len(want.splitlines()) > 3


# ---- 5. refusals
def test_refusals(tmp_path):
    bed, _ = region_beds(tmp_path, "nofilt")["stranded"]
    table = str(tmp_path / "t.tsv")
    loc = ["--localize", bed, "--localize-out", table]
    def refused(argv, status, word, run=modkit_amd.pileup):
        with pytest.raises(modkit_amd.MkpError) as e:
            run(argv)
        assert e.value.status == status and word in str(e.value), (argv, str(e.value))
    base = [BC, str(tmp_path / "x.bed"), "--no-filtering"]
    refused([os.path.join(FIX, "duplex_modcalls_sort.bam"), "-o", str(tmp_path / "h.bed"), "--cpg", "--ref", REF] + loc, INVALID,
            "unexpected argument '--localize'", run=modkit_amd.pileup_hemi)
    refused([BC, str(tmp_path / "parts"), "--no-filtering", "--partition-tag", "HP"] + loc, INVALID, "--partition-tag")
    refused(base + ["--gpus-world", "2", "--gpus-rank", "0"] + loc, UNSUPPORTED, "--gpus-world")
    refused(base + ["--plan-only"] + loc, INVALID, "--plan-only")
    refused(base + ["--localize-only", "--bgzf"] + loc, INVALID, "--localize-only")
    refused(base + ["--localize-only", "--bedgraph"] + loc, INVALID, "--localize-only")
    refused(base + ["--localize-only"], INVALID, "need --localize")
    refused(base + ["--localize-window", "9"], INVALID, "need --localize")
    refused(base + ["--localize-stranded", "same"], INVALID, "need --localize")
    refused(base + ["--localize-stranded-features", "."], INVALID, "need --localize")
    refused(base + ["--localize-out", table], INVALID, "need --localize")
    refused(base + loc + ["--localize-window", "100001"], UNSUPPORTED, "--localize-window")
    # no region left after the contig filter: none of the BED's contigs is in the BAM header
    nowhere = tmp_path / "nowhere.bed"; nowhere.write_text("chrNone\t5\t9\nchrNone2\t1\t2\n")
    refused(base + ["--localize", str(nowhere), "--localize-out", table], INVALID, "valid regions")
    assert not os.path.exists(table)
