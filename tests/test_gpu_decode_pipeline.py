"""GPU: the slot decoder's two-deep software pipeline (mkp_decode_slots: B(s), A(s + 1), C(s) per iteration, A(0) in front of the loop, the
last step's byte stored behind it) on one small directed BAM built with the builders of tests/cigar_edge_cases.py, one shard, focus
positions from --include-bed so that every directed read's slot count is exact:

  slot counts 0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193 and 257 per read (prologue only, prologue and drain, steady state, a last step of
  one lane), both strands, layouts m (one code), h_m and hm (two codes);
  reads of one reference base per op over 1 500 ops whose focus positions come in clusters, so that step s + 1 lies in the next CIGAR
  window and two or more windows on from step s, with the window edge 0, 1, 33 and 63 bases off a step edge;
  a deletion and a ref-skip over a whole step between two steps with calls (on and off the step grid); a step of matches without a listed
  call between two steps with calls, and the reverse (the reference has no C / G there and the ops are `=`);
  reads whose last step holds a lane or two in front of a trailing insertion / soft clip, or behind a deletion (a CIGAR whose query length
  exceeds SEQ — the decoder's `q >= L` guard — is refused by both packers and cannot be written here);
  reads of five steps with `N` bases (the SEQ byte path), with an op of 4 096 (the 32-bit CIGAR words), with a delta list that runs past its
  base (coverage only) and without calls, in each of the three layouts;
  the kinds interleaved along the contig under a layer of ordinary reads.  (Waves are launched longest read first, so what shares a
  workgroup is decided by length: the five-step reads with `N` bases, with a run-over list, without calls and the plain ones are all 302 bases long, three of a kind,
  so any four neighbours among them are of two kinds or more.)

Flag set A is --include-bed with a fixed --filter-threshold: device rows == the column model, device text == the oracle's, the fused
decoder's text == MKP_FUSED=0's.  Flag set B adds --ignore h (the collapsed code's ML byte; outside the column model's scope): device text
== the oracle's == MKP_FUSED=0's.  Under both, rerun(1) then rerun(0, fetch) on the resident shard return the first pass's digest.  Every
comparison is exact."""
import os
import random
import subprocess

import pytest

import cigar_edge_cases as cases
import column_model as cm
import modkit_amd

pytestmark = pytest.mark.gpu

SLOT_COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257]
LAYOUTS3 = ("m", "h_m", "hm")
REF_LEN = 70_000


def _span(ops):
    return cases.ref_span(ops)


def specs():
    """[(kind, name, ops, layout, reverse, [(a, b) focus spans relative to the read's start], no-C/G spans, record edit or None)]"""
    out = []
    # exact slot counts
    for n in SLOT_COUNTS:
        for layout in LAYOUTS3:
            for rev in (False, True):
                ops = [(n // 2 + 10, "M"), (2, "D"), (3, "I"), (n - n // 2 + 20, "M")]
                out.append(("count", "n%03d" % n, ops, layout, rev, [(7, 7 + n)] if n else [], [], None))
    # one reference base per op: the window of 256 ops ends (lead - 1) % 64 bases off a step edge; clustered focus spans
    for lead in (1, 2, 34, 64):
        for pat, layout in ((2, "m"), (4, "h_m")):
            if pat == 2:
                tail = [(1, "D") if i % 2 == 0 else (1, "M") for i in range(1500)]
            else:
                tail = [(1, "I") if i % 4 == 0 else (1, "D") if i % 4 == 2 else (1, "M") for i in range(1500)]
            ops = [(lead, "M")] + tail
            s = _span(ops)
            focus = [(0, 192), (450, 514)] + ([(1100, 1164)] if s > 1300 else []) + [(s - 69, s - 5)]
            out.append(("window", "w%02d_%d" % (lead, pat), ops, layout, (lead + pat) % 4 == 2, focus, [], None))
    # a gap over a whole step
    for gap in "DN":
        out.append(("gap", "g64" + gap, [(64, "M"), (64, gap), (64, "M")], "m", False, [(0, 192)], [], None))
        out.append(("gap", "g64r" + gap, [(64, "M"), (64, gap), (64, "M")], "h_m", True, [(0, 192)], [], None))
        out.append(("gap", "g150" + gap, [(70, "M"), (150, gap), (80, "M")], "hm", gap == "N", [(0, 300)], [], None))
    # a step without a listed call between two with calls, and the reverse
    for rev in (False, True):
        out.append(("nocall", "mid%d" % rev, [(192, "=")], "m" if rev else "h_m", rev, [(0, 192)], [(64, 128)], None))
        out.append(("nocall", "ends%d" % rev, [(192, "=")], "hm" if rev else "m", rev, [(0, 192)], [(0, 64), (128, 192)], None))
    # the last step: a lane or two, in front of a trailing insertion and soft clip / behind a deletion
    out.append(("tail", "t_is", [(130, "M"), (4, "I"), (6, "S")], "m", False, [(0, 130)], [], None))
    out.append(("tail", "t_isr", [(130, "M"), (4, "I"), (6, "S")], "h_m", True, [(0, 130)], [], None))
    out.append(("tail", "t_d1", [(5, "S"), (128, "M"), (3, "D"), (1, "M")], "hm", False, [(0, 132)], [], None))
    out.append(("tail", "t_d1r", [(5, "S"), (128, "M"), (3, "D"), (1, "M")], "m", True, [(0, 132)], [], None))

    # special reads of five steps
    def seqn(rec):
        start, flag, cigar, seq, mm, ml = rec
        seq = list(seq)
        spots = [k for k, b in enumerate(seq) if b in "AT"]      # (neither strand's tags count A or T: MM / ML stay as written)
        for k in spots[3::len(spots) // 7]:
            seq[k] = "N"
        assert "N" in seq
        return start, flag, cigar, "".join(seq), mm, ml

    def runover(rec):
        start, flag, cigar, seq, mm, ml = rec
        tags = []
        for t in mm.split(";")[:-1]:
            head, last = t.rsplit(",", 1)
            tags.append("%s,%d" % (head, int(last) + len(seq)))
        return start, flag, cigar, seq, ";".join(tags) + ";", ml

    def callless(rec):
        start, flag, cigar, seq, mm, ml = rec
        return start, flag, cigar, seq, ";".join(t.split(",")[0] for t in mm.split(";")[:-1]) + ";", []

    five = [(150, "M"), (3, "D"), (2, "I"), (150, "M")]
    wide = [(100, "M"), (4096, "N"), (220, "M")]
    for k, layout in enumerate(LAYOUTS3):
        rev = k % 2 == 1
        out.append(("seqn", "sn_" + layout, five, layout, rev, [(0, 303)], [], seqn))
        out.append(("wide", "wd_" + layout, wide, layout, not rev, [(0, 100), (2000, 2064), (4196, 4416)], [], None))
        out.append(("runover", "ro_" + layout, five, layout, rev, [(0, 303)], [], runover))
        out.append(("callless", "cl_" + layout, five, layout, not rev, [(0, 303)], [], callless))
        out.append(("plain", "pl_" + layout, five, layout, rev, [(0, 303)], [], None))
    # the kinds interleaved along the contig
    by_kind = {}
    for sp in out:
        by_kind.setdefault(sp[0], []).append(sp)
    order, queues = [], list(by_kind.values())
    while any(queues):
        for qu in queues:
            if qu:
                order.append(qu.pop(0))
    return order


def build(prefix):
    r = random.Random(91)
    ref = cases.make_ref(r, REF_LEN)
    L = cases.Layer(92, ref)
    at, focus, placed = 300, [], []
    for kind, name, ops, layout, rev, spans, bare, edit in specs():
        start = at
        at += _span(ops) + 23
        for a, b in bare:
            for p in range(start + a, start + b):
                ref[p] = "AT"[p % 2] if ref[p] in "CG" else ref[p]
        L.add(ops, layout, rev, start=start, name="%s_%s%s" % (name, layout, "r" if rev else "f"))
        if edit:
            L.records[-1] = edit(L.records[-1])
        focus += [(start + a, start + b) for a, b in spans]
        placed.append((L.names[-1], kind, start, _span(ops), sum(b - a for a, b in spans)))
    assert at + 2000 < REF_LEN, at
    L.background(200, at, 2)      # ordinary reads over everything: columns of several reads, their slot counts whatever the spans give
    c = cases.Case("decode_pipeline", "pipe", "".join(ref), L, prefix)
    c.focus = sorted(focus)
    c.placed = placed
    c.focus_bed = prefix + "_focus.bed"
    with open(c.focus_bed, "w") as f:
        for a, b in c.focus:
            f.write("%s\t%d\t%d\n" % (c.contig, a, b))
    return c


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    c = build(str(tmp_path_factory.mktemp("decode_pipeline") / "pipe"))
    c.walked, c.oracle = {}, {}
    return c


def flag_sets(case):
    thr = ["--filter-threshold", str(cases.THRESHOLD)]
    return [["--include-bed", case.focus_bed] + thr, ["--include-bed", case.focus_bed, "--ignore", "h"] + thr]


def _device(bam, out, flags, fused=True):
    old = {k: os.environ.get(k) for k in ("MKP_FUSED", "MKP_HOST_INGEST")}
    try:
        os.environ.pop("MKP_FUSED", None)
        os.environ.pop("MKP_HOST_INGEST", None)
        if not fused:
            os.environ["MKP_FUSED"] = "0"
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


def test_the_bam_holds_the_shapes(case):
    """the builder's own bookkeeping: every slot count on both strands and in the three layouts, reads of every kind, and the kinds
    interleaved along the contig"""
    covered = set()
    for a, b in case.focus:
        covered.update(range(a, b))
    seen = set()
    for name, kind, start, span, n_focus in case.placed:
        n_sl = sum(1 for p in range(start, start + span) if p in covered)
        if kind == "count":
            assert n_sl == n_focus == int(name[1:4]), name
            seen.add((n_sl, name[-1], name[5:-1]))
        elif kind != "wide":
            assert n_sl >= n_focus > 128, name
    assert seen == {(n, s, lay) for n in SLOT_COUNTS for s in "fr" for lay in LAYOUTS3}
    kinds = [k for _, k, _, _, _ in case.placed]
    assert set(kinds) == {"count", "window", "gap", "nocall", "tail", "seqn", "wide", "runover", "callless", "plain"}
    assert sum(1 for a, b in zip(kinds[:40], kinds[1:41]) if a != b) >= 30
    by_name = dict(zip(case.read_names, case.records))
    # launch order is by read length: the 302-base reads, three of a kind, cannot fill a workgroup of four with one kind
    same_len = [k for (nm, k, _, _, _) in case.placed if len(by_name[nm][3]) == 302]
    assert len(same_len) == 12 and set(same_len) == {"seqn", "runover", "callless", "plain"}
    assert all(same_len.count(k) <= 3 for k in ("seqn", "runover", "callless", "plain"))
    assert all("N" in by_name["sn_%s_%s%s" % (lay, lay, "fr"[k % 2])][3] for k, lay in enumerate(LAYOUTS3))


def test_rows_equal_model_oracle_and_unfused(oracle_bin, case, tmp_path):
    flags = flag_sets(case)[0]
    thr = cases.THRESHOLD
    if thr not in case.walked:
        case.walked[thr] = cm.walk(case.records, thr)
    want = cm.pileup(case.records, case.ref, threshold=thr, bed=[(a, b, ".") for a, b in case.focus], walked=case.walked[thr])
    assert len(want) > 5_000
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    out = str(tmp_path / "dev.bed")
    fused = _device(case.bam, out, flags, True)
    got = cm.read_bedmethyl(out).get(case.contig, {})
    d = cm.first_difference(got, want)
    if d:
        over = [(case.read_names[i], start, flag, k, op, w) for i, start, flag, k, op, w in cm.covering(case.records, d[0][0])]
        raise AssertionError("device vs model: first difference at (pos, strand, code) %r: device %r, model %r %s; reads over it (name, "
                             "start, flag, op index, op, window): %s" % (d[0], d[1], d[2], cm.COUNTS, over))
    assert fused == ora, "device text differs from the oracle's"
    unfused = _device(case.bam, str(tmp_path / "dev0.bed"), flags, False)
    assert fused == unfused, "fused slot decoder differs from MKP_FUSED=0"


def test_ignore_h_equals_oracle_and_unfused(oracle_bin, case, tmp_path):
    flags = flag_sets(case)[1]
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    assert len(ora.splitlines()) > 5_000
    fused = _device(case.bam, str(tmp_path / "dev.bed"), flags, True)
    assert fused == ora, "device text differs from the oracle's"
    unfused = _device(case.bam, str(tmp_path / "dev0.bed"), flags, False)
    assert fused == unfused, "fused slot decoder differs from MKP_FUSED=0"


@pytest.mark.parametrize("fi", [0, 1], ids=["plain", "ignore_h"])
def test_one_shard_and_relaunch(oracle_bin, case, tmp_path, fi, monkeypatch):
    """one shard; the wide reads take the 32-bit words; rerun(1) then rerun(0, fetch) return the first pass's rows"""
    monkeypatch.delenv("MKP_FUSED", raising=False)
    monkeypatch.delenv("MKP_HOST_INGEST", raising=False)
    flags = flag_sets(case)[fi]
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    ora_path = str(tmp_path / "ora_rows.bed")
    open(ora_path, "w").write(ora)
    digest = modkit_amd.rows_digest(modkit_amd.read_bedmethyl(ora_path))
    dev = str(tmp_path / "dev.bed")
    ctx = modkit_amd.Context(device=0)
    try:
        rep = ctx.pileup_run([case.bam, dev] + flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and open(dev).read() == ora
        got = ctx.read_flags()
        # (a read that ends in front of the first focus span or begins behind the last one is never fetched)
        assert len(case.records) - 4 <= len(got) <= len(case.records)
        assert sum(1 for f in got if f & modkit_amd.READ_WIDE_CIGAR) == sum(1 for nm in case.read_names if nm.startswith("wd_")) == 3
        ctx.rerun(1)
        assert modkit_amd.rows_digest(modkit_amd.rows_to_numpy(ctx.rerun(0, fetch=True))) == digest
    finally:
        ctx.close()
