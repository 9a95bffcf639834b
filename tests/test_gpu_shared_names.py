"""GPU: kept records that share a read name inside one interval — find_shared_names / plan_name_owners (mkp_plan.hpp) and mkp_dup_restore /
mkp_dup_events / mkp_dup_apply (mkp_slots.hip) — against the name-keyed cache of the per-base model (tests/column_model.py, shared_walk)
and against the oracle, on the directed BAMs of tests/shared_name_cases.py: the 64-lane batches and segment ends of mkp_dup_events,
consumers of 255 to 513 CIGAR ops, owners and consumers of different strands, tags and status, ownership by file order, `N` ops,
deletions and focus positions, one name in two partition keys, and owners that disagree.

Every BAM runs without a focus (mkp_pileup_tiles), under --cpg (the slot pipeline, mkp_cover_reads), with every position a slot
(--include-bed of the whole contig) and under --cpg --combine-strands; unfiltered, with --filter-threshold 0.7, with -i 1000 (which
cuts the groups) and with --region; `ownership` also with --shard-bp and with a BED of several spans, `status` also under --edge-filter.  Each flag set runs on the
indexed file (device ingest: the planner fetches the members' CIGARs from the device) and the unindexed one (host packer), at the
default tile and with --tile 256, on the default path and with MKP_FUSED=0 (not under an edge filter, where the fused decoder is never
used).

The order of the assertions says where a failure is: device rows == model (with the reads over the first differing position), then
device text == oracle text.  No row and no column is left out.  The floors of shared_name_cases.FLOORS are the model's own numbers
(tests/test_column_model.py holds them equal); they are conditions on the input.
"""
import os
import subprocess

import pytest

import cigar_edge_cases as cases
import column_model as cm
import modkit_amd
import shared_name_cases as sn

pytestmark = pytest.mark.gpu

PARAMS = [(name, fi) for name in sorted(sn.FLOORS) if name != "partition" for fi in range(len(sn.FLOORS[name]))]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            case = sn.BUILDERS[name](str(tmp_path_factory.mktemp(name) / name))
            case.walked = {}
            cache[name] = case
        return cache[name]
    return get


def _oracle(oracle_bin, bam, out, flags):
    p = subprocess.run([oracle_bin, "pileup", bam, out] + cases.oracle_flags(flags), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-400:]
    return open(out).read()


def _device(args, fused=True):
    old = os.environ.get("MKP_FUSED")
    try:
        if fused:
            os.environ.pop("MKP_FUSED", None)
        else:
            os.environ["MKP_FUSED"] = "0"
        modkit_amd.pileup(args)
    finally:
        if old is None:
            os.environ.pop("MKP_FUSED", None)
        else:
            os.environ["MKP_FUSED"] = old


def _first_text_diff(a, b):
    al, bl = a.splitlines(), b.splitlines()
    for i in range(max(len(al), len(bl))):
        x = al[i] if i < len(al) else "<none>"
        y = bl[i] if i < len(bl) else "<none>"
        if x != y:
            return "row %d\n  %s\n  %s (%d vs %d rows)" % (i, x, y, len(al), len(bl))
    return None


def _check_rows(case, path, want, what):
    got = cm.read_bedmethyl(path) if os.path.exists(path) else {}
    assert set(got) <= {case.contig}
    d = cm.first_difference(got.get(case.contig, {}), want)
    if d:
        over = [(case.read_names[i], start, flag, k, op, w) for i, start, flag, k, op, w in cm.covering(case.records, d[0][0])]
        raise AssertionError("%s vs model: first difference at (pos, strand, code) %r: device %r, model %r %s; reads over it "
                             "(name, start, flag, op index, op, window): %s" % (what, d[0], d[1], d[2], cm.COUNTS, over))


def _paths(case, flags):
    """(bam, --tile flags, fused) of every run of one flag set"""
    t256 = ["--tile", str(sn.TILE)]
    for bam, tile in ((case.bam, []), (case.bam, t256), (case.bam_unindexed, []), (case.bam_unindexed, t256)):
        for fused in ((True,) if "--edge-filter" in flags else (True, False)):
            yield bam, tile, fused


def _model_then_oracle(oracle_bin, case, flags, want, tmp_path):
    ora = {}
    for bam, tile, fused in _paths(case, flags):
        if bam not in ora:
            ora[bam] = _oracle(oracle_bin, bam, str(tmp_path / "ora.bed"), flags)
        what = "%s, %s, %s, %s" % (os.path.basename(bam), " ".join(flags[-6:] + tile), "default path" if fused else "MKP_FUSED=0", case.name)
        out = str(tmp_path / "dev.bed")
        _device([bam, out] + flags + tile, fused)
        _check_rows(case, out, want, what)
        d = _first_text_diff(open(out).read(), ora[bam])
        assert d is None, "%s vs oracle: %s" % (what, d)


@pytest.mark.parametrize("name,fi", PARAMS)
def test_device_equals_model_then_oracle(oracle_bin, built, tmp_path, name, fi):
    case = built(name)
    flags = sn.flag_sets(case)[fi]
    want, numbers, mixed = sn.model_rows(case, flags, case.walked)
    assert numbers == sn.FLOORS[name][fi] and not mixed
    assert numbers[0] > 100 and numbers[1] > 0 and (numbers[2] > 0 or name == "status")
    assert numbers[3] > 0 or name not in ("bases_strands", "ownership")
    _model_then_oracle(oracle_bin, case, flags, want, tmp_path)


def test_rebuilt_lists_survive_a_relaunch(oracle_bin, built, tmp_path):
    """mkp_dup_apply points a consumer's header at its rebuilt list; mkp_dup_restore must point it at its own events again before the
    decoders of the next pass run: a second pass over the resident shard, and a third, give the first pass's rows."""
    case = built("batches")
    for fi in (0, 5, 10):           # no focus; --cpg with a threshold; every position a slot under -i 1000
        flags = sn.flag_sets(case)[fi]
        want, numbers, _ = sn.model_rows(case, flags, case.walked)
        assert numbers[2] > 200
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


@pytest.mark.parametrize("shape", sorted(sn.MIXED_SHAPES))
def test_owners_that_disagree_are_refused_and_their_neighbours_run(oracle_bin, tmp_path, shape):
    """MKP_E_UNSUPPORTED exactly where the model reports a record whose owners differ in status or observed codes; the shapes next to
    those (the same tags; an owner change where status and codes agree; one interval; two bad owners) run and equal the model."""
    case = sn.mixed(shape, str(tmp_path / shape))
    want, numbers, mixed = sn.model_rows(case, case.flags, {})
    assert bool(mixed) == sn.MIXED[shape] and numbers[1] > 0
    if not mixed:
        _model_then_oracle(oracle_bin, case, case.flags, want, tmp_path)
        return
    for bam, tile, fused in _paths(case, case.flags):
        with pytest.raises(modkit_amd.MkpError) as e:
            _device([bam, str(tmp_path / "dev.bed")] + case.flags + tile, fused)
        assert e.value.status == -3 and "read name" in str(e.value), (bam, tile, fused)


@pytest.mark.parametrize("fi", range(len(sn.FLOORS["partition"])))
def test_partition_keys_share_one_name_cache(built, tmp_path, fi):
    """--partition-tag HP: each key's file == the model's rows for that key.  The reference keeps ONE read cache for all keys
    (pileup/mod.rs:745), asked by name alone: a record of key 2 whose name a record of key 1 owns is answered from that record."""
    case = built("partition")
    flags = sn.flag_sets(case)[fi]
    want, numbers, mixed = sn.model_rows(case, flags, case.walked)
    assert numbers == sn.FLOORS["partition"][fi] and not mixed and numbers[1] > 0 and numbers[2] > 0
    names = {1: "1.bed", 2: "2.bed", None: "ungrouped.bed"}
    assert all(len(want[k]) > 20 for k in names)
    for bam, tile, fused in _paths(case, flags):
        out_dir = str(tmp_path / ("parts_%s_%d_%d" % (os.path.basename(bam), len(tile), fused)))
        _device([bam, out_dir, "--partition-tag", "HP"] + flags + tile, fused)
        assert sorted(f for f in os.listdir(out_dir) if f.endswith(".bed")) == sorted(names.values())
        for key, f in names.items():
            what = "key %s, %s, %s, %s" % (key, os.path.basename(bam), " ".join(flags[-6:] + tile), "default path" if fused else "MKP_FUSED=0")
            _check_rows(case, os.path.join(out_dir, f), want[key], what)
