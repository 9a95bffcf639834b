"""GPU: the pileup kernels' CIGAR -> reference mapping and column tallies against the per-base model (tests/column_model.py), and
against the oracle, on the directed BAMs of tests/cigar_edge_cases.py: reads on the edges of the 256-op window, the four-op lane quads,
the 64-op chunks, the 16 / 32-bit scan switch and the 64-slot steps; spliced reads with `N` ops of 1 kb to 400 kb; D / N / I ops and CpG
pairs on tile, interval, region and shard seams.

Every BAM runs with every position a slot (--include-bed of the whole contig), --motif C 0, --cpg, --cpg --combine-strands and without a
focus (the dense tile kernel); the indexed file (device ingest) and the unindexed one (host packer), each at the default tile and with
--tile 256 (the two large BAMs: indexed + default tile and unindexed + --tile 256 only); each through the default path (fused slot decoder for classes 0 / 1, mkp_cover_reads + event decoders for 2-4) and with MKP_FUSED=0
(every class through the event decoders and mkp_cover_reads, on the BAM words' form of the slot walks' CIGAR window, cigwin_map).  The order of the assertions says where a failure is: device rows == model
column by column, then device text == oracle text.  No row and no column is left out.

The floors were computed on the CPU from the model and are constants here: rows per flag set, rows with a deletion, rows with
N_diff > 0, the tiles the longest spliced read spans, the rows inside introns (which only the unspliced layer gives).
"""
import bisect
import os
import subprocess

import pytest

import cigar_edge_cases as cases
import column_model as cm
import modkit_amd

pytestmark = pytest.mark.gpu

N_FLAG_SETS = {"window_edges": 5, "scan_switch": 5, "slot_steps": 5, "spliced": 5, "seams": 15}
# ingest (indexed: device ingest, unindexed: host packer) x tile (default, --tile 256) runs as a full cross on the small BAMs; the two
# large ones run the pairs indexed + default tile and unindexed + --tile 256 only, to keep the file's time down: a limit of this file
PAIRED_ONLY = ("scan_switch", "spliced")
PARAMS = [(name, fi) for name in sorted(N_FLAG_SETS) for fi in range(N_FLAG_SETS[name])]

# (rows, rows with N_delete > 0, rows with N_diff > 0) the model gives per flag set, less a tenth (at least 1): what each run must at least hold
FLOORS = {
    "window_edges": [(32704, 802, 170), (46211, 1155, 105), (11162, 251, 27), (13076, 359, 36), (32704, 802, 170)],
    "scan_switch": [(153057, 17700, 2272), (209267, 25356, 1681), (52043, 5906, 419), (65168, 8860, 601), (153057, 17700, 2272)],
    "slot_steps": [(4403, 1089, 589), (4655, 1188, 415), (1466, 363, 119), (979, 368, 122), (4403, 1089, 589)],
    "spliced": [(63160, 840, 14065), (60464, 773, 8554), (18070, 242, 2621), (10477, 247, 2521), (63160, 840, 14065)],
    "seams": [(62685, 30955, 5799), (62685, 30955, 5799), (62685, 30955, 5799), (71399, 33403, 3565), (3982, 1071, 694), (71399, 33403, 3565), (21006, 10377, 1156), (1404, 366, 216), (21006, 10377, 1156), (15669, 8361, 1219), (773, 315, 207), (15669, 8361, 1219), (62685, 30955, 5799), (4300, 1153, 1109), (62685, 30955, 5799)],
}
SPLICED_MIN_TILES = 1_400        # the longest spliced read spans more than this many tiles of 256 positions (the model: 1 586)
SPLICED_INTRON_ROWS = 44_000          # --include-bed rows at positions inside the inner part of some spliced read's intron (the model: 49 868); unspliced reads give all of them


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            case = cases.BUILDERS[name](str(tmp_path_factory.mktemp(name) / name))
            case.walked = {}
            cache[name] = case
        return cache[name]
    return get


def _model(case, flags, records=None):
    kw = cases.model_kwargs(case, flags)
    if records is not None:
        return cm.pileup(records, case.ref, **kw)
    thr = kw["threshold"]
    if thr not in case.walked:
        case.walked[thr] = cm.walk(case.records, thr)
    return cm.pileup(case.records, case.ref, walked=case.walked[thr], **kw)


def _oracle(oracle_bin, bam, out, flags):
    p = subprocess.run([oracle_bin, "pileup", bam, out] + cases.oracle_flags(flags), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-400:]
    return open(out).read()


def _device(bam, out, flags, fused):
    old = os.environ.get("MKP_FUSED")
    try:
        if fused:
            os.environ.pop("MKP_FUSED", None)
        else:
            os.environ["MKP_FUSED"] = "0"
        modkit_amd.pileup([bam, out] + flags)
    finally:
        if old is None:
            os.environ.pop("MKP_FUSED", None)
        else:
            os.environ["MKP_FUSED"] = old
    return open(out).read()


def _first_text_diff(a, b):
    al, bl = a.splitlines(), b.splitlines()
    for i in range(max(len(al), len(bl))):
        x = al[i] if i < len(al) else "<none>"
        y = bl[i] if i < len(bl) else "<none>"
        if x != y:
            return "row %d\n  %s\n  %s (%d vs %d rows)" % (i, x, y, len(al), len(bl))
    return None


def _check_rows(case, path, want, what):
    got = cm.read_bedmethyl(path).get(case.contig, {})
    d = cm.first_difference(got, want)
    if d:
        over = [(case.read_names[i], start, flag, k, op, w) for i, start, flag, k, op, w in cm.covering(case.records, d[0][0])]
        raise AssertionError("%s vs model: first difference at (pos, strand, code) %r: device %r, model %r %s; reads over it "
                             "(name, start, flag, op index, op, window): %s" % (what, d[0], d[1], d[2], cm.COUNTS, over))


@pytest.mark.parametrize("name,fi", PARAMS)
def test_device_equals_model_then_oracle(oracle_bin, built, tmp_path, name, fi):
    case = built(name)
    flags = cases.flag_sets(case)[fi]
    want = _model(case, flags)
    rows, with_del, with_diff = FLOORS[name][fi]
    assert len(want) >= rows and sum(1 for v in want.values() if v[4]) >= with_del and sum(1 for v in want.values() if v[6]) >= with_diff
    assert len(want) > 100
    t256 = ["--tile", str(cases.TILE)]
    runs = [(case.bam, []), (case.bam_unindexed, t256)]
    if name not in PAIRED_ONLY:
        runs += [(case.bam, t256), (case.bam_unindexed, [])]
    ora = {}
    for bam, tile in runs:
        if bam not in ora:
            ora[bam] = _oracle(oracle_bin, bam, str(tmp_path / "ora.bed"), flags)
        for fused in (True, False):
            what = "%s, %s, %s, %s" % (os.path.basename(bam), " ".join(flags[-6:] + tile), "default path" if fused else "MKP_FUSED=0", name)
            out = str(tmp_path / "dev.bed")
            dev = _device(bam, out, flags + tile, fused)
            _check_rows(case, out, want, what)
            d = _first_text_diff(dev, ora[bam])
            assert d is None, "%s vs oracle: %s" % (what, d)


def test_directed_cigars_reach_both_decoders(built):
    """What the runs above rest on: every op count, every edge op on every edge index, is there for the fused slot decoder (classes
    0 / 1) and for the event decoders (classes 2-4)."""
    case = built("window_edges")
    fused, events = cases.op_counts_by_decoder(case)
    assert set(cases.WINDOW_OP_COUNTS) <= fused and set(cases.WINDOW_OP_COUNTS) <= events
    for index in cases.EDGE_INDEXES[0] + cases.EDGE_INDEXES[1]:
        f, e = cases.ops_at_by_decoder(case, index)
        assert set("IDNP") <= f and set("IDNP") <= e, (index, f, e)


def test_spliced_floor_and_relaunch(oracle_bin, built, tmp_path):
    """The spliced BAM tests what it says: a read over more than 100 tiles, rows inside introns that come from the unspliced layer
    alone; and a re-launch on the resident shard returns the first pass's rows."""
    case = built("spliced")
    spans = [cases.ref_span(cigar) for (_, _, cigar, _, _, _), nm in zip(case.records, case.read_names) if nm.startswith("sp")]
    assert max(spans) // cases.TILE > SPLICED_MIN_TILES
    flags = cases.flag_sets(case)[0]
    want = _model(case, flags)
    unspliced = [rec for rec, nm in zip(case.records, case.read_names) if not nm.startswith("sp")]
    alone = _model(case, flags, records=unspliced)

    merged = []
    for a, b in sorted(case.introns):
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    starts = [a for a, _ in merged]

    def inside(rows):
        out = {}
        for k, v in rows.items():
            i = bisect.bisect_right(starts, k[0]) - 1
            if i >= 0 and k[0] < merged[i][1]:
                out[k] = v
        return out
    assert inside(want) == inside(alone) and len(inside(want)) >= SPLICED_INTRON_ROWS > 0
    ora_path, dev = str(tmp_path / "ora.bed"), str(tmp_path / "dev.bed")
    ora = _oracle(oracle_bin, case.bam, ora_path, flags)
    digest = modkit_amd.rows_digest(modkit_amd.read_bedmethyl(ora_path))
    ctx = modkit_amd.Context(device=0)
    try:
        rep = ctx.pileup_run([case.bam, dev] + flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and open(dev).read() == ora
        _check_rows(case, dev, want, "resident shard, first pass")
        assert modkit_amd.rows_digest(modkit_amd.rows_to_numpy(ctx.rerun(0, fetch=True))) == digest
        assert modkit_amd.rows_digest(modkit_amd.rows_to_numpy(ctx.rerun(2, fetch=True))) == digest
    finally:
        ctx.close()
