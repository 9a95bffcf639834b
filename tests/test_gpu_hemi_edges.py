"""GPU: the pileup-hemi kernels (SPARSE decode per group + mkp_merge_duplex, the general decoder, the HEMI instantiation of the tile
kernel with its partner search, mkp_hemi_failed_reads) against the per-base duplex model (tests/hemi_model.py), and against the oracle,
on the directed BAMs of tests/hemi_edge_cases.py: group sizes on the merge's 64-entry rank windows, partners in the next lane batch and
across tile / interval / region / shard seams, CIGARs on the 128-op and 64-op windows, reads on the 4096-base SPARSE step, failed
records over 1, 2 and 5 intervals.

Every BAM runs under --cpg, --motif CG 1, --motif CCGG 0, --motif GC 0 and --cpg --combine-mods, unfiltered or with
--filter-threshold 0.7 (partner_edges also with -i 500, --region, --include-bed and --shard-bp 3000; failed_records also with -i 500);
the indexed file (device ingest) and the unindexed one (host packer), each at the default tile and with --tile 256.  The order of the
assertions says where a failure is: device rows == model column by column, then device text == oracle text.  No row and no column is
left out.  The floors of hemi_edge_cases.FLOORS (the model's own numbers less a tenth) keep every run from going empty.
"""
import subprocess

import pytest

import hemi_edge_cases as hc
import hemi_model as hm
import modkit_amd

pytestmark = pytest.mark.gpu

N_FLAG_SETS = {name: len(floors) for name, floors in hc.FLOORS.items()}
PARAMS = [(name, fi) for name in sorted(N_FLAG_SETS) for fi in range(N_FLAG_SETS[name])]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            case = hc.BUILDERS[name](str(tmp_path_factory.mktemp(name) / name))
            case.parsed, case.loaded = hm.parse(case.records), {}
            cache[name] = case
        return cache[name]
    return get


def _model(case, flags):
    kw = hc.model_kwargs(case, flags)
    thr = kw["threshold"]
    if thr not in case.loaded:
        case.loaded[thr] = hm.load(case.records, thr, case.parsed)
    return hm.pileup_hemi(case.records, case.ref, loaded=case.loaded[thr], **kw)


def _oracle(oracle_bin, bam, out, flags):
    p = subprocess.run([oracle_bin, "pileup-hemi", bam, "-o", out] + hc.oracle_flags(flags), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-400:]
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
    got = hm.read_hemi_bed(path)
    assert set(got) <= {case.contig}
    d = hm.first_difference(got.get(case.contig, {}), want)
    if d:
        over = [(case.read_names[i], start, flag, k, op, w) for i, start, flag, k, op, w in hm.covering(case.records, d[0][0])]
        raise AssertionError("%s vs model: first difference at (pos, pattern, base) %r: device %r, model %r %s; reads over it "
                             "(name, start, flag, op index, op, window): %s" % (what, d[0], d[1], d[2], hm.COUNTS, over))


@pytest.mark.parametrize("name,fi", PARAMS)
def test_device_equals_model_then_oracle(oracle_bin, built, tmp_path, name, fi):
    case = built(name)
    flags = hc.flag_sets(case)[fi]
    want = _model(case, flags)
    rows, with_del, with_nocall, not_canonical, mixed = hc.FLOORS[name][fi]
    cols = {}
    for pos, pattern, base in want:
        cols.setdefault(pos, set()).add((pattern, base))
    assert len(want) >= rows and sum(1 for v in want.values() if v[5]) >= with_del and sum(1 for v in want.values() if v[8]) >= with_nocall
    assert sum(1 for k in want if k[1] != "-,-") >= not_canonical and sum(1 for c in cols.values() if len(c) > 1) >= mixed
    assert len(want) > (hc.FAILED_MIN_ROWS if name == "failed_records" else 100)
    ora = _oracle(oracle_bin, case.bam, str(tmp_path / "ora.bed"), flags)      # (the two files hold the same records)
    for bam in (case.bam, case.bam_unindexed):
        for tile in ([], ["--tile", str(hc.TILE)]):
            what = "%s, %s, %s" % (bam.rsplit("/", 1)[-1], " ".join(flags[:-2] + tile), name)
            out = str(tmp_path / "dev.bed")
            modkit_amd.pileup_hemi([bam, "-o", out] + flags + tile)
            _check_rows(case, out, want, what)
            d = _first_text_diff(open(out).read(), ora)
            assert d is None, "%s vs oracle: %s" % (what, d)


def _code(v):
    v = int(v)
    return "-" if v == 0 else str(v & 0x7fffffff) if v >> 31 else chr(v)


@pytest.mark.parametrize("name", ["failed_records", "partner_edges"])
def test_relaunch_on_the_resident_shard_returns_the_same_rows(oracle_bin, built, tmp_path, name):
    """mkp_hemi_failed_reads writes a failed record's NoCalls into the record's own event slice, which the next pass reads again:
    re-launches on the resident shard must leave the first pass's rows.  mkp_shard_rerun hands out no rows of a pileup-hemi plan
    (tests/test_gpu_parity_hemi.py pins that), so the rows after the re-launches are read with mkp_hemi_shard_run over the same
    intervals, and compared with the model column by column."""
    case = built(name)
    flags = [f for f in hc.flag_sets(case) if "-i" in f and "--cpg" in f and "--shard-bp" not in f and "--include-bed" not in f][0]
    kw = hc.model_kwargs(case, flags)
    want = _model(case, flags)
    ora_path, dev = str(tmp_path / "ora.bed"), str(tmp_path / "dev.bed")
    ora = _oracle(oracle_bin, case.bam, ora_path, flags)
    ctx = modkit_amd.Context(device=0)
    try:
        rep = ctx.pileup_hemi_run([case.bam, "-o", dev] + flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and rep.n_rows == len(want)
        _check_rows(case, dev, want, "resident shard, first pass")
        assert open(dev).read() == ora
        ctx.rerun(2)                                         # the hemi kernels twice more on the resident shard
        starts = [a for a, _, _ in hm.intervals(case.ref, None, kw["interval"], kw["motif"], True)]
        r = ctx.hemi_shard_run(hm.negative_strand_position(0, kw["motif"]), starts)
        got = {}
        for i in range(len(r["pos"])):
            key = (int(r["pos"][i]), "%s,%s" % (_code(r["pattern_pos"][i]), _code(r["pattern_neg"][i])), chr(r["primary_base"][i]))
            assert key not in got
            got[key] = (int(r["n_valid"][i]), want.get(key, ("", ""))[1]) + tuple(int(r[f][i]) for f in ("count", "n_canonical", "n_other_pattern", "n_delete", "n_fail", "n_diff", "n_nocall"))
        d = hm.first_difference(got, want)
        assert d is None, "after the re-launches: first difference at (pos, pattern, base) %r: device %r, model %r %s" % (d + (hm.COUNTS,))
    finally:
        ctx.close()
