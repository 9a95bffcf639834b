"""GPU: the fused slot decoder visits only the focus slots of a read's own strand (MkpWork.ent_off / n_ent, the slot-entry lists of
mkp_plan.hpp); the bytes of the stream it no longer writes stay BLANK from the prefill.  One small directed BAM built with the builders of
tests/cigar_edge_cases.py over a reference this test writes: it holds no CG but the ones placed here, so that under --cpg --ref every
read's slots are known — the C of a CpG has the '+' rule only, the G the '-' rule only.

  own-strand slot counts 0, 1, 63, 64, 65, 128 and 129 per read on both strands, in two shapes: `out` — the read's first and its last
  global slot are the other strand's (stream bytes that are never written), k own slots among 2 k + 1; `in` — first and last are its own,
  k among 2 k - 1;
  a deletion and a ref-skip over slots of both strands, and reads whose ref-skips cover other-strand slots only (the unfused decoder flags
  such a read MKP_VF_GAPS, the fused one no longer does);
  reads with `N` bases, with an op of 4 096 bases and without calls, over CpGs three bases apart (100 own slots in 300 bases);
  reads the event decoders take (implicit-mode and ChEBI tags) in the same shard, and a layer of ordinary reads over everything.

Every comparison is exact: device text == the oracle's == MKP_FUSED=0's == MKP_STRAND_SLOTS=0's."""
import os
import random
import subprocess

import pytest

import cigar_edge_cases as cases
import modkit_amd

pytestmark = pytest.mark.gpu

OWN_COUNTS = [0, 1, 63, 64, 65, 128, 129]
LAYOUTS3 = ("m", "h_m", "hm")
FLANK = 12


def specs():
    """[(kind, name, ops, layout, reverse, read start relative to its region, [C positions of the region's CpGs, relative], region length, edit)]"""
    out = []
    for k in OWN_COUNTS:
        for rev in (False, True):
            for shape in ("out", "in"):
                if shape == "in" and k == 0:
                    continue
                cs = [FLANK + 4 * j for j in range(k + 1 if shape == "out" else k)]     # the region's CpGs, four bases apart
                if shape == "out":      # forward: G_0 .. G_k; reverse: C_0 .. C_k
                    a, b = (cs[0] + 1, cs[k] + 2 + 10) if not rev else (cs[0] - 10, cs[k] + 1)
                else:                   # forward: C_0 .. C_(k-1); reverse: G_0 .. G_(k-1)
                    a, b = (cs[0] - 10, cs[k - 1] + 1) if not rev else (cs[0] + 1, cs[k - 1] + 2 + 10)
                n = b - a
                ops = [(n, "M")] if n < 8 else [(n // 2, "M"), (3, "I"), (n - n // 2, "M")]
                layout = LAYOUTS3[(k + rev) % 3]
                out.append(("count", "k%03d%s" % (k, shape), ops, layout, rev, a, cs, cs[-1] + 2 + FLANK, None))
    # a deletion / a ref-skip over slots of both strands
    cs = [FLANK + 4 * j for j in range(40)]
    for gap in "DN":
        for rev in (False, True):
            out.append(("gap", "g40" + gap, [(60, "M"), (40, gap), (70, "M")], "m" if rev else "h_m", rev, 2, cs, 200, None))
    # ref-skips over other-strand slots only: CpGs eight apart, a two-base N over every G (forward) / every C (reverse)
    cs = [FLANK + 8 * j for j in range(12)]
    for rev in (False, True):
        ops, pos = [], 0
        for c in cs:
            lo = c + 1 if not rev else c - 1
            ops += [(lo - pos, "M"), (2, "N")]
            pos = lo + 2
        ops.append((9, "M"))
        out.append(("skip_other", "so", ops, "hm" if rev else "m", rev, 0, cs, pos + 9 + FLANK, None))

    def seqn(rec):
        start, flag, cigar, seq, mm, ml = rec
        seq = list(seq)
        spots = [i for i, b in enumerate(seq) if b in "AT"]      # (neither strand's tags count A or T: MM / ML stay as written)
        for i in spots[3::max(1, len(spots) // 7)]:
            seq[i] = "N"
        assert "N" in seq
        return start, flag, cigar, "".join(seq), mm, ml

    def callless(rec):
        start, flag, cigar, seq, mm, ml = rec
        return start, flag, cigar, seq, ";".join(t.split(",")[0] for t in mm.split(";")[:-1]) + ";", []

    dense = [FLANK + 3 * j for j in range(100)]
    five = [(150, "M"), (3, "D"), (2, "I"), (150, "M")]
    wide_cs = [FLANK + 4 * j for j in range(30)] + [2000 + 4 * j for j in range(20)] + [4200 + 4 * j for j in range(50)]
    for i, layout in enumerate(LAYOUTS3):
        rev = i % 2 == 1
        out.append(("seqn", "sn", five, layout, rev, FLANK - 3, dense, 340, seqn))
        out.append(("callless", "cl", five, layout, not rev, FLANK - 3, dense, 340, callless))
        out.append(("wide", "wd", [(100, "M"), (4096, "N"), (220, "M")], layout, rev, FLANK - 2, wide_cs, 4450, None))
    # reads of the event decoders and mkp_cover_reads in the same shard
    for i, layout in enumerate(("m_dot", "chebi", "h_m_dot", "m_dot")):
        out.append(("events", "ev", [(90, "M"), (2, "D"), (100, "M")], layout, i % 2 == 1, 5, [FLANK + 4 * j for j in range(45)], 230, None))
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
    r = random.Random(171)
    plan, at, cpgs = [], 300, []
    for kind, name, ops, layout, rev, a, cs, length, edit in specs():
        plan.append((kind, name, ops, layout, rev, at + a, edit))
        cpgs += [at + c for c in cs]
        at += length + 23
    ref_len = at + 2500
    ref = [r.choice("ACGT") for _ in range(ref_len)]
    placed = set(cpgs)
    for c in placed:
        ref[c], ref[c + 1] = "C", "G"
    for p in range(ref_len - 1):        # no CG but the placed ones (a G turned into A or T makes no new one)
        if ref[p] == "C" and ref[p + 1] == "G" and p not in placed:
            ref[p + 1] = "AT"[p % 2]
    assert {p for p in range(ref_len - 1) if ref[p] == "C" and ref[p + 1] == "G"} == placed
    L = cases.Layer(172, ref)
    info = []
    for kind, name, ops, layout, rev, start, edit in plan:
        L.add(ops, layout, rev, start=start, name="%s_%s%s" % (name, layout, "r" if rev else "f"))
        if edit:
            L.records[-1] = edit(L.records[-1])
        info.append((L.names[-1], kind, start, cases.ref_span(ops), rev, ops))
    L.background(200, at, 2)      # ordinary reads over everything
    c = cases.Case("strand_slots", "strands", "".join(ref), L, prefix)
    c.cpgs, c.info = placed, info
    c.oracle = {}
    return c


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("strand_slots") / "strands"))


THR = ["--filter-threshold", str(cases.THRESHOLD)]


def cpg_flag_sets(case):
    base = ["--cpg", "--ref", case.fa] + THR
    return {"cpg": base, "combine": base + ["--combine-strands"], "ignore_h": base + ["--ignore", "h"]}


KNOBS = ("MKP_FUSED", "MKP_STRAND_SLOTS", "MKP_HOST_INGEST")


def _device(bam, out, flags, **env):
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
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
    """the builder's own bookkeeping, by brute force over the reference: every own-strand count on both strands and in both shapes, whose
    first / last global slot is whose, and what the ref-skips cover"""
    seen = set()
    for name, kind, start, span, rev, ops in case.info:
        slots = [(p, "+") for p in range(start, start + span) if p in case.cpgs] + [(p, "-") for p in range(start, start + span) if p - 1 in case.cpgs]
        slots.sort()
        own = "-" if rev else "+"
        n_own = sum(1 for _, s in slots if s == own)
        if kind == "count":
            k, shape = int(name[1:4]), name[4:].split("_")[0]
            assert n_own == k, name
            if shape == "out":
                assert len(slots) == 2 * k + 1 and slots[0][1] != own and slots[-1][1] != own, name
            else:
                assert len(slots) == 2 * k - 1 and slots[0][1] == own and slots[-1][1] == own, name
            seen.add((k, shape, rev))
        elif kind in ("gap", "skip_other"):
            p, skipped = start, []
            for n, op in ops:
                if op in "DN":
                    skipped += [s for q, s in slots if p <= q < p + n]
                if op in "MDN=X":
                    p += n
            if kind == "gap":
                assert skipped.count("+") >= 9 and skipped.count("-") >= 9, name
            else:
                assert len(skipped) == 12 and own not in skipped and n_own == 12, name
        elif kind in ("seqn", "callless"):
            assert n_own >= 95 and len(slots) >= 190, name
    assert seen == {(k, sh, rev) for k in OWN_COUNTS for sh in ("out", "in") for rev in (False, True) if not (sh == "in" and k == 0)}
    kinds = {k for _, k, _, _, _, _ in case.info}
    assert kinds == {"count", "gap", "skip_other", "seqn", "callless", "wide", "events"}
    by_name = dict(zip(case.read_names, case.records))
    assert all("N" in by_name[nm][3] for nm, k, _, _, _, _ in case.info if k == "seqn")
    assert all(by_name[nm][5] == [] for nm, k, _, _, _, _ in case.info if k == "callless")


@pytest.mark.parametrize("which", ["cpg", "combine", "ignore_h"])
def test_equals_oracle_unfused_and_knob(oracle_bin, case, tmp_path, which):
    """the same shard holds fused reads and reads of the event decoders (one kind of them with implicit-mode tags)"""
    flags = cpg_flag_sets(case)[which]
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    assert len(ora.splitlines()) > 1_500
    dev = _device(case.bam, str(tmp_path / "dev.bed"), flags)
    assert dev == ora, "device text differs from the oracle's"
    assert _device(case.bam, str(tmp_path / "dev0.bed"), flags, MKP_FUSED="0") == dev, "fused slot decoder differs from MKP_FUSED=0"
    assert _device(case.bam, str(tmp_path / "dev1.bed"), flags, MKP_STRAND_SLOTS="0") == dev, "strand lists differ from MKP_STRAND_SLOTS=0"


def test_both_rules_everywhere_stays_on_all(oracle_bin, case, tmp_path):
    """--include-bed alone: every position is a slot with both rules, no strand list is shorter than `all`"""
    flags = ["--include-bed", case.bed] + THR
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    assert len(ora.splitlines()) > 10_000
    assert _device(case.bam, str(tmp_path / "dev.bed"), flags) == ora


def _run(ctx, case, out, flags):
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        rep = ctx.pileup_run([case.bam, out] + flags)
    finally:
        os.environ.update({k: v for k, v in old.items() if v is not None})
    return rep, open(out).read()


@pytest.mark.parametrize("which", ["cpg", "combine"])
def test_small_tiles(oracle_bin, case, tmp_path, which):
    """tiles of 32 slots: reads cross tiles, and tiles begin on a slot of either strand — the other strand's for half of the reads over it"""
    flags = cpg_flag_sets(case)[which]
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    ctx = modkit_amd.Context(device=0, tile_positions=128)
    try:
        rep, text = _run(ctx, case, str(tmp_path / "dev.bed"), flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and text == ora
    finally:
        ctx.close()


def test_prefill_per_shard(oracle_bin, case, tmp_path):
    """three or more shards on one context: the stream buffer is reused, the bytes no read writes must be BLANK again in every shard"""
    flags = cpg_flag_sets(case)["cpg"] + ["--interval-size", "4000"]
    ctx = modkit_amd.Context(device=0)
    try:
        rep1, one = _run(ctx, case, str(tmp_path / "one.bed"), flags + ["--shard-bytes", str(1 << 40)])
        repn, many = _run(ctx, case, str(tmp_path / "many.bed"), flags + ["--shard-bytes", "1"])
        assert rep1.n_shards == 1 and repn.n_shards >= 3
        assert many == one
        # and once more in the order that leaves a larger shard's bytes under the small ones
        rep1, again = _run(ctx, case, str(tmp_path / "again.bed"), flags + ["--shard-bytes", str(1 << 40)])
        assert again == one
    finally:
        ctx.close()
    assert one == _oracle(oracle_bin, case, tmp_path, cpg_flag_sets(case)["cpg"])


@pytest.mark.parametrize("which", ["cpg", "ignore_h"])
def test_relaunch(oracle_bin, case, tmp_path, which):
    """rerun(1) then rerun(0, fetch) on the resident shard return the first pass's rows: a fused read writes the same bytes on every pass"""
    flags = cpg_flag_sets(case)[which]
    ora = _oracle(oracle_bin, case, tmp_path, flags)
    ora_path = str(tmp_path / "ora_rows.bed")
    open(ora_path, "w").write(ora)
    digest = modkit_amd.rows_digest(modkit_amd.read_bedmethyl(ora_path))
    ctx = modkit_amd.Context(device=0)
    try:
        rep, text = _run(ctx, case, str(tmp_path / "dev.bed"), flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and text == ora
        ctx.rerun(1)
        assert modkit_amd.rows_digest(modkit_amd.rows_to_numpy(ctx.rerun(0, fetch=True))) == digest
    finally:
        ctx.close()
