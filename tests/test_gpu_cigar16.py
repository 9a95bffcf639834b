"""GPU: the slot decoder's two CIGAR paths — the 16-bit array (mkp_cigar_pack.hpp: four ops per lane from one 8-byte load) for reads
whose ops are all 4 095 bases or shorter, the 32-bit words for every other read — on one directed BAM built with the builders of
tests/cigar_edge_cases.py:

  reads of 1, 3, 4, 5, 255, 256, 257, 511, 512, 513 and 1 025 ops (lane-quad, window and prefetch edges);
  one op of exactly 4 095 (the read stays on the 16-bit path) and of exactly 4 096 (it leaves it), each at the first, a middle and the
  last op index, as a match, and in the middle as a deletion and a ref-skip;
  a read with a 100 kb intron; reads of both kinds interleaved in one shard, forward and reverse, for both fused decode classes (and the
  4 095 / 4 096 reads once more for the event decoders, which never see the 16-bit array);
  two records without a CIGAR (the packers give them one soft clip: 50 bases, and 5 000 — an op that does not fit).

Each run on the device ingest and with MKP_HOST_INGEST=1 (the host packer).  The packer's flag says which path every read took
(Context.read_flags); device rows == the column model, device text == the oracle's, the fused decoder's text == MKP_FUSED=0's; a
re-launch on the resident shard returns the first pass's rows."""
import os
import random
import subprocess

import pytest

import cigar_edge_cases as cases
import column_model as cm
import modkit_amd

pytestmark = pytest.mark.gpu

OP_COUNTS = [1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1025]
FUSED_LAYOUTS = (("m", False), ("h_m", True))        # decode classes 0 and 1, one strand each (the second round swaps the strands)
DROPPED = 4 | 256 | 512 | 1024 | 2048                # what the pileup never keeps


def build(prefix):
    r = random.Random(71)
    ref = cases.make_ref(r, 330_000)
    L = cases.Layer(72, ref)
    k = [0]

    def add(ops, wide, layouts=FUSED_LAYOUTS, start=None):
        """the read for every layout; the name says which path it is meant to take (w: 32-bit words, c: 16-bit)"""
        assert wide == any(n > 4095 for n, _ in ops)
        for layout, rev in layouts:
            rev = rev ^ (k[0] % 2 == 1)
            L.add(ops, layout, rev, start=start, name="%s%05d" % ("w" if wide else "c", len(L.records)))
        k[0] += 1
    for n in OP_COUNTS:
        add(cases.gapped_cigar(L.r, n), False)
    both = ((4095, False), (4096, True))              # the two kinds alternate along the contig: one shard holds them interleaved
    for at in (0, 4, 8):                                  # first, middle and last op of nine (match slots)
        for n, wide in both:
            ops = cases.gapped_cigar(L.r, 9)
            ops[at] = (n, "M")
            add(ops, wide)
            if at == 4:
                add(ops, wide, layouts=cases.BOTH_DECODERS[2:])
    for gap in "DN":
        for n, wide in both:
            ops = cases.gapped_cigar(L.r, 9)
            ops[3] = (n, gap)
            add(ops, wide)
    # and in a CIGAR of more than one window: the long op in the first window, in the second, and as the very last op
    for at in (2, 300, 512):
        for n, wide in both:
            ops = cases.gapped_cigar(L.r, 513)
            ops[at] = (n, "M")
            add(ops, wide)
    add([(70, "M"), (100_000, "N"), (60, "M"), (2, "D"), (70, "M")], True, start=200_000)
    add([(70, "M"), (4_000, "N"), (60, "M"), (2, "D"), (70, "M")], False, start=200_010)
    L.background(199_900, 200_400, 4)
    L.background(300_000, 300_400, 4)
    # records without a CIGAR: mapped, with bases and tags (the threshold sampler takes them, the pileup does not)
    for j, n in enumerate((50, 5000)):
        start, flag, _, seq, mm, ml = cases.make_read(L.r, ref, 1_000 + 3_000 * j, [(n, "M")], "m", j == 1, 9000 + j)
        L.records.append((start, flag, [], seq, mm, ml))
        L.names.append("nocigar%d" % j)
        L.layouts.append(None)
    L.flagged_copies()
    return cases.Case("cigar16", "c16", "".join(ref), L, prefix)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    c = build(str(tmp_path_factory.mktemp("cigar16") / "cigar16"))
    c.aligned = [rec for rec in c.records if rec[2]]       # what the column model walks (it has no CIGAR-less records)
    c.walked, c.oracle = {}, {}
    return c


def flag_sets(case):
    thr = ["--filter-threshold", str(cases.THRESHOLD)]
    return [["--include-bed", case.bed] + thr, ["--cpg", "--ref", case.fa] + thr]


def _device(bam, out, flags, fused=True, host_ingest=False):
    old = {k: os.environ.get(k) for k in ("MKP_FUSED", "MKP_HOST_INGEST")}
    try:
        os.environ.pop("MKP_FUSED", None)
        os.environ.pop("MKP_HOST_INGEST", None)
        if not fused:
            os.environ["MKP_FUSED"] = "0"
        if host_ingest:
            os.environ["MKP_HOST_INGEST"] = "1"
        modkit_amd.pileup([bam, out] + flags)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return open(out).read()


def _oracle(oracle_bin, case, tmp_path, flags):
    key = " ".join(flags)
    if key not in case.oracle:
        out = str(tmp_path / "ora.bed")
        p = subprocess.run([oracle_bin, "pileup", case.bam, out] + flags, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-400:]
        case.oracle[key] = open(out).read()
    return case.oracle[key]


def _model(case, flags):
    kw = cases.model_kwargs(case, flags)
    thr = kw["threshold"]
    if thr not in case.walked:
        case.walked[thr] = cm.walk(case.aligned, thr)
    return cm.pileup(case.aligned, case.ref, walked=case.walked[thr], **kw)


@pytest.mark.parametrize("host_ingest", [False, True], ids=["device_ingest", "host_ingest"])
@pytest.mark.parametrize("fi", [0, 1], ids=["every_position", "cpg"])
def test_rows_equal_model_oracle_and_unfused(oracle_bin, case, tmp_path, fi, host_ingest):
    flags = flag_sets(case)[fi]
    want = _model(case, flags)
    assert len(want) > 10_000 if fi == 0 else len(want) > 300
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    out = str(tmp_path / "dev.bed")
    fused = _device(case.bam, out, flags, True, host_ingest)
    got = cm.read_bedmethyl(out).get(case.contig, {})
    d = cm.first_difference(got, want)
    if d:
        over = [(case.read_names[case.records.index(case.aligned[i])], start, flag, k, op, w)
                for i, start, flag, k, op, w in cm.covering(case.aligned, d[0][0])]
        raise AssertionError("device vs model: first difference at (pos, strand, code) %r: device %r, model %r %s; reads over it (name, "
                             "start, flag, op index, op, window): %s" % (d[0], d[1], d[2], cm.COUNTS, over))
    assert fused == ora, "device text differs from the oracle's"
    unfused = _device(case.bam, str(tmp_path / "dev0.bed"), flags, False, host_ingest)
    assert fused == unfused, "fused slot decoder differs from MKP_FUSED=0"


@pytest.mark.parametrize("host_ingest", [False, True], ids=["device_ingest", "host_ingest"])
def test_each_read_takes_its_path_and_relaunch(oracle_bin, case, tmp_path, host_ingest, monkeypatch):
    """the packer's flag per kept read == what the read's name says; compact and wide reads of both strands and both fused layouts sit in
    the one shard; rerun(1) then rerun(0, fetch) return the first pass's rows"""
    monkeypatch.delenv("MKP_FUSED", raising=False)
    if host_ingest:
        monkeypatch.setenv("MKP_HOST_INGEST", "1")
    else:
        monkeypatch.delenv("MKP_HOST_INGEST", raising=False)
    flags = flag_sets(case)[0]
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    ora_path = str(tmp_path / "ora_rows.bed")
    open(ora_path, "w").write(ora)
    digest = modkit_amd.rows_digest(modkit_amd.read_bedmethyl(ora_path))
    kept = [(nm, rec, lay) for nm, rec, lay in zip(case.read_names, case.records, case.layouts) if not rec[1] & DROPPED and rec[2] and rec[3]]
    dev = str(tmp_path / "dev.bed")
    ctx = modkit_amd.Context(device=0)
    try:
        rep = ctx.pileup_run([case.bam, dev] + flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and open(dev).read() == ora
        got = ctx.read_flags()
        assert len(got) == len(kept)
        seen = set()
        for f, (nm, rec, lay) in zip(got, kept):
            wide = bool(f & modkit_amd.READ_WIDE_CIGAR)
            assert bool(f & 1) == bool(rec[1] & 16), nm
            assert wide == any(n > 4095 for n, _ in rec[2]), (nm, rec[2][:12])
            if nm[0] in "wc":
                assert wide == (nm[0] == "w"), nm
                if cases.LAYOUTS[lay][1] in cases.FUSED_CLASSES:
                    seen.add((wide, bool(rec[1] & 16), lay))
        assert seen == {(w, rv, lay) for w in (False, True) for rv in (False, True) for lay in ("m", "h_m")}
        # the two kinds are interleaved in file order, not one block each
        kinds = [bool(f & modkit_amd.READ_WIDE_CIGAR) for f in got]
        assert sum(1 for a, b in zip(kinds, kinds[1:]) if a != b) >= 8
        ctx.rerun(1)
        assert modkit_amd.rows_digest(modkit_amd.rows_to_numpy(ctx.rerun(0, fetch=True))) == digest
    finally:
        ctx.close()


@pytest.mark.parametrize("host_ingest", [False, True], ids=["device_ingest", "host_ingest"])
def test_records_without_a_cigar(oracle_bin, case, tmp_path, host_ingest):
    """an estimated threshold: the sampler packs the CIGAR-less records (one soft clip each, 50 bases and 5 000) next to the others, on both
    ingests; the pileup itself never keeps them"""
    assert sum(1 for rec in case.records if not rec[2] and rec[3]) == 2
    flags = ["--cpg", "--ref", case.fa]
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    assert len(ora.splitlines()) > 300
    assert _device(case.bam, str(tmp_path / "dev.bed"), flags, True, host_ingest) == ora
    assert _device(case.bam, str(tmp_path / "dev0.bed"), flags, False, host_ingest) == ora
