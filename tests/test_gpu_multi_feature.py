"""GPU: the reads the fused slot decoder never takes — several primary bases in one read, tags on the read's '-' strand (two features on
one column), `N`-base tags, 8 tags and 12 (base, code) pairs in a run, and every read once an edge filter is set — against the per-base
model (tests/column_model.py) and against the oracle, on the directed BAMs of tests/multi_feature_cases.py.  These reads go through the
general event decoder (decode class 4), the duplex layouts (`C+m?;G-m?`, `C+h?;C+m?;G-h?;G-m?`: classes 5 / 6) through one SPARSE decode
per group and mkp_merge_duplex, classes 2 / 3 and, under an edge filter, 0 / 1 through the FAST and SPARSE event decoders; then
mkp_cover_reads with its overflow list, the overflow loops of mkp_pileup_stream and the event path of mkp_pileup_tiles.

Every BAM runs with every position a slot (--include-bed of the whole contig), --cpg, --cpg --combine-strands and without a focus (the
dense tile kernel), unfiltered or with --filter-threshold 0.7; event_merge and many_tags also with --combine-mods, event_merge with
-i 1000 and --region, edge_filter under each of its trims, plain and inverted.  Each flag set runs on the indexed file (device ingest)
and the unindexed one (host packer), each at the default tile and with --tile 256; and all of that again with MKP_FUSED=0, which changes
only the decoder of the class 0 / 1 neighbours — except under an edge filter, where the fused decoder is never used and the second run
would be the first one again.

The order of the assertions says where a failure is: device rows == model column by column (with the reads over the first differing
position), then device text == oracle text.  No row and no column is left out.  The floors of multi_feature_cases.FLOORS are the
model's own numbers (tests/test_column_model.py holds them equal): rows, rows with N_diff > 0, aligned bases with two features of one
read, calls removed by the edge filter.
"""
import os
import subprocess

import pytest

import cigar_edge_cases as cases
import column_model as cm
import modkit_amd
import multi_feature_cases as mf

pytestmark = pytest.mark.gpu

PARAMS = [(name, fi) for name in sorted(mf.FLOORS) for fi in range(len(mf.FLOORS[name]))]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            case = mf.BUILDERS[name](str(tmp_path_factory.mktemp(name) / name))
            case.walked, case.parsed = {}, {}
            cache[name] = case
        return cache[name]
    return get


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


def _check_rows(case, path, want, what, who="device"):
    got = cm.read_bedmethyl(path)
    assert set(got) <= {case.contig}
    d = cm.first_difference(got.get(case.contig, {}), want)
    if d:
        over = [(case.read_names[i], start, flag, k, op, w) for i, start, flag, k, op, w in cm.covering(case.records, d[0][0])]
        raise AssertionError("%s vs model: first difference at (pos, strand, code) %r: %s %r, model %r %s; reads over it "
                             "(name, start, flag, op index, op, window): %s" % (what, d[0], who, d[1], d[2], cm.COUNTS, over))


@pytest.mark.parametrize("name,fi", PARAMS)
def test_device_equals_model_then_oracle(oracle_bin, built, tmp_path, name, fi):
    case = built(name)
    flags = mf.flag_sets(case)[fi]
    want, numbers = mf.model_rows(cm, case, flags, case.walked, case.parsed)
    assert all(10 * got >= 9 * floor for got, floor in zip(numbers, mf.FLOORS[name][fi])), (numbers, mf.FLOORS[name][fi])
    assert len(want) > 100 and numbers[1] > 0
    assert numbers[3] > 0 or "--edge-filter" not in flags
    t256 = ["--tile", str(mf.TILE)]
    ora, same_as_model = {}, {}
    for bam, tile in ((case.bam, []), (case.bam, t256), (case.bam_unindexed, []), (case.bam_unindexed, t256)):
        if bam not in ora:
            path = str(tmp_path / "ora.bed")
            ora[bam] = _oracle(oracle_bin, bam, path, flags)
            rows = cm.read_bedmethyl(path)
            same_as_model[bam] = set(rows) <= {case.contig} and rows.get(case.contig, {}) == want
        for fused in ((True,) if "--edge-filter" in flags else (True, False)):
            what = "%s, %s, %s, %s" % (os.path.basename(bam), " ".join(flags[-6:] + tile), "default path" if fused else "MKP_FUSED=0", name)
            out = str(tmp_path / "dev.bed")
            dev = _device(bam, out, flags + tile, fused)
            # device rows == model: text equal to an oracle text whose rows are the model's says so; anything else is parsed and compared
            if dev != ora[bam] or not same_as_model[bam]:
                _check_rows(case, out, want, what)
            d = _first_text_diff(dev, ora[bam])
            assert d is None, "%s vs oracle: %s" % (what, d)


def test_overflow_list_survives_a_relaunch(oracle_bin, built, tmp_path):
    """mkp_cover_reads writes a read's overflow list over the front of its own event slice: a second pass over the resident shard, and a
    third after it, must each give the first pass's rows (the decoders write the events again before every pass)."""
    case = built("event_merge")
    for fi in (0, 1):           # every position a slot; --cpg
        flags = mf.flag_sets(case)[fi]
        want, numbers = mf.model_rows(cm, case, flags, case.walked, case.parsed)
        assert numbers[2] > 10_000
        ora_path, dev = str(tmp_path / "ora.bed"), str(tmp_path / "dev.bed")
        ora = _oracle(oracle_bin, case.bam, ora_path, flags)
        digest = modkit_amd.rows_digest(modkit_amd.read_bedmethyl(ora_path))
        ctx = modkit_amd.Context(device=0)
        try:
            rep = ctx.pileup_run([case.bam, dev] + flags + ["--shard-bytes", str(1 << 40)])
            assert rep.n_shards == 1
            _check_rows(case, dev, want, "resident shard, first pass")
            assert open(dev).read() == ora
            for nth in ("second", "third"):       # (rerun(n) launches the pass n times and fetches the last one's rows)
                assert modkit_amd.rows_digest(modkit_amd.rows_to_numpy(ctx.rerun(1, fetch=True))) == digest, "%s pass" % nth
        finally:
            ctx.close()
