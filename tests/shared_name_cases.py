"""Directed modBAMs for kept records that share a read NAME inside one interval.  The reference answers every later record of a name from
the call map of the record it asked about first (its per-interval ReadCache is keyed by name, read_cache.rs:24-43, 232-355); the device
works out the owners on the host (find_shared_names, plan_name_owners, mkp_plan.hpp) and rebuilds the later records' event lists with
mkp_dup_restore / mkp_dup_events / mkp_dup_apply (mkp_slots.hip).  These BAMs go where the fuzz (a copy, a shifted copy or a split half,
always of the owner's strand and tags) does not: the 64-lane batches and the segment ends of mkp_dup_events, consumers of several CIGAR
windows, owners and consumers of different strands, tags and status, ownership decided by file order, `N` ops, deletions and focus
positions, names that span partition keys, and owners that disagree.

One contig of 6 kb per BAM, a few dozen records, written with the writers of tests/bamfuzz.py, indexed and unindexed.  The records of a
shared name carry the reference's own bases except where a SNP or an `N` is placed; every BAM also holds plain `C+m?` / `C+h?;C+m?` reads
with unique names over the same columns.  ML bytes are the pattern {250, 10, 140} of tests/multi_feature_cases.py (every other code 2):
no call is near a tie.  Every builder asserts its shape from the records as written; where the shape is about who owns a name, from the
owners tests/column_model.py's loop arrives at.
"""
import random

import column_model as cm
import multi_feature_cases as mf
from bamfuzz import aux_bc, aux_i, aux_z, bam_header, bam_record, bgzf_write, write_bai
from cigar_edge_cases import make_ref, ref_span

THRESHOLD = mf.THRESHOLD
TILE = mf.TILE
CONTIG_LEN = 6_000
INTERVAL = 1_000
REGION = (1_450, 4_550)
BATCH_EVENTS = (1, 63, 64, 65, 128, 129)
LONG_OP_COUNTS = (255, 256, 257, 513)


class Case:
    """The records as written (file order: by start, then as added), their names and partition keys, and the files."""

    def __init__(self, name, contig, ref, added, prefix):
        order = sorted(range(len(added)), key=lambda i: added[i][1][0])
        self.name, self.contig, self.ref, self.seams = name, contig, ref, {}
        self.read_names = [added[i][0] for i in order]
        self.records = [added[i][1] for i in order]
        self.keys = [added[i][2] for i in order]
        self.bam, self.bam_unindexed, self.fa, self.bed = prefix + ".bam", prefix + "_noidx.bam", prefix + ".fa", prefix + ".bed"
        data, idx = bam_header([(contig, len(ref))]), []
        for (start, flag, cigar, seq, mm, ml), qname, key in zip(self.records, self.read_names, self.keys):
            aux = aux_z("MM", mm) + aux_bc("ML", ml) + (aux_i("HP", key) if key is not None else b"")
            rec = bam_record(0, start, flag, qname, cigar, seq, aux)
            idx.append((0, start, ref_span(cigar), flag, len(data), len(rec)))
            data += rec
        offs = bgzf_write(self.bam, bytes(data))             # indexed: device ingest
        write_bai(self.bam + ".bai", 1, offs, idx)
        bgzf_write(self.bam_unindexed, bytes(data))          # unindexed: host packer
        with open(self.fa, "w") as f:
            f.write(">%s\n" % contig)
            for i in range(0, len(ref), 60):
                f.write(ref[i:i + 60] + "\n")
        with open(self.bed, "w") as f:                       # every position of the contig, both strands
            f.write("%s\t0\t%d\n" % (contig, len(ref)))

    def index(self, name, nth=0):
        return [i for i, nm in enumerate(self.read_names) if nm == name][nth]


class Book:
    """Collects the records of one BAM."""

    def __init__(self, seed, c_every=0, edits=()):
        self.r = random.Random(seed)
        self.ref = make_ref(self.r, CONTIG_LEN)
        if c_every:                       # a C-rich contig: a `C+m?` owner has a call on every c_every-th base
            for p in range(0, CONTIG_LEN, c_every):
                self.ref[p] = "C"
        for p, text in edits:
            self.ref[p:p + len(text)] = text
        self.added = []

    def add(self, name, start, cigar, layout="m", reverse=False, force=None, only=None, key=None, spoil=None, flag=0):
        """only: list calls at exactly these reference positions ('clip': on the clipped bases alone); spoil: 'short_ml' | 'runaway', tags the reference cannot parse"""
        bases = mf.true_bases(self.ref, start, ref_span(cigar))
        bases.update(force or {})
        keep = None
        if only == "clip":                # calls on bases that have no reference position only: a good record without one event
            keep = lambda t, tag, cand: [c for c in cand if c[2] is None]
        elif only is not None:
            keep = mf.keep_plan({p: 3 for p in only})
        rec, _, _ = mf.make_read(self.r, self.ref, start, cigar, layout, reverse, 1000 + len(self.added), flag, force=bases, keep=keep)
        if spoil == "short_ml":
            rec = rec[:5] + (rec[5][:-1],)
        elif spoil == "runaway":          # a delta list that runs past the read's last C
            head, _, rest = rec[4].partition(";")
            rec = rec[:4] + (head + ",%d;" % (len(rec[3]) + 5) + rest, rec[5] + [200])
        else:
            assert spoil is None
        self.added.append((name, rec, key))
        return rec

    def background(self, lo, hi, depth=2, mean=300, reverse=None, keys=(None,)):
        r, k0 = self.r, len(self.added)
        for k in range(max(1, (hi - lo) * depth // mean)):
            n = r.randrange(mean // 2, mean * 3 // 2)
            start = r.randrange(lo, max(lo + 1, hi - n))
            a = r.randrange(20, n - 20)
            gap = r.choice([(r.randrange(1, 8), "D"), (r.randrange(1, 8), "I"), None])
            cigar = [(n, "M")] if gap is None else [(a, "M"), gap, (n - a, "M")]
            rev = r.random() < 0.5 if reverse is None else reverse
            rec, _, _ = mf.make_read(r, self.ref, start, cigar, r.choice(mf.PLAIN), rev, 5000 + k0 + k)
            self.added.append(("bg%05d" % (k0 + k), rec, r.choice(keys)))

    def finish(self, name, contig, prefix):
        c = Case(name, contig, "".join(self.ref), self.added, prefix)
        assert len(c.ref) == CONTIG_LEN and 10 <= len(c.records) <= 150, len(c.records)
        shared = {nm for nm in c.read_names if c.read_names.count(nm) > 1}
        assert shared and any(nm not in shared for nm in c.read_names)
        return c


def listed(rec):
    """The reference positions of a record's calls per tag, from the record as written: [(tag head, {positions})]; a '.' tag calls every
    base of its kind"""
    start, flag, cigar, seq, mm, ml = rec
    L, at, p, q = len(seq), {}, start, 0
    for n, op in cigar:
        if op in "M=X":
            for k in range(n):
                at[L - 1 - (q + k) if flag & 16 else q + k] = p + k
        if op in "MDN=X":
            p += n
        if op in "MIS=X":
            q += n
    tags, fwd = mf.written_calls(rec)
    out = []
    for head, mode, fw in tags:
        if mode == ".":
            fw = {i for i, b in enumerate(fwd) if b == head[0]}
        out.append((head, {at[i] for i in fw if i in at}))
    return out


def call_positions(rec):
    return {p for _, ps in listed(rec) for p in ps}


def states(rec):
    """{reference position: index into SEQ | 'D' | 'N'} of a record"""
    start, flag, cigar, seq, mm, ml = rec
    out, p, q = {}, start, 0
    for n, op in cigar:
        for k in range(n if op in "M=XDN" else 0):
            out[p + k] = q + k if op in "M=X" else op
        if op in "MDN=X":
            p += n
        if op in "MIS=X":
            q += n
    return out


def owners(case, **kw):
    """{record index: [(interval start, owner's index, owner is good, codes)]} as the model's loop finds them"""
    report = cm.new_report()
    cm.pileup(case.records, case.ref, names=case.read_names, report=report, **kw)
    return report["asked"]


# ---------------------------------------------------------------------------------------------------------------------------------
def batches(prefix):
    """1. the 64-lane batches and the segment ends of mkp_dup_events: foreign segments of 1 / 63 / 64 / 65 / 128 / 129 owner events, and
    under -i of 0 events of an owner that has some (all in the interval in front, or all in the one behind); a good owner without one
    event; an owner list that ends on the 64th event of a segment and one
    that goes on into the next segment; under -i an owner event on p_lo - 1, p_lo, p_hi - 1 and p_hi; a consumer of three segments: its
    own, a foreign one, its own."""
    B = Book(201, c_every=3, edits=[(3_999, "CC")])
    at = 60
    for n in BATCH_EVENTS:                   # (a) the owner lists exactly n calls; the consumer, five bases on, lies over all of them
        if at % INTERVAL + 440 > INTERVAL:   # (inside one interval, so that the segment holds n events under -i as well)
            at = (at // INTERVAL + 1) * INTERVAL + 30
        cs = [p for p in range(at + 9, at + 400) if B.ref[p] == "C"][:n]
        B.add("batch%03d" % n, at, [(420, "M")], only=cs)
        B.add("batch%03d" % n, at + 5, [(400, "M")])
        at += 230
    # (b) `ends`: the owner's list is 64 events long.  `goes_on`: 64 events in front of the seam at 3000 and five behind it, where the
    # name belongs to another record (`taker`: in file order the first, it sits in an `N` op until just in front of the seam, so the
    # owner is asked first in [2000, 3000) and the taker in [3000, 4000)).  `no_events`: a good owner whose calls all lie on clipped bases
    seam = 3 * INTERVAL
    front = [p for p in range(seam - 200, seam) if B.ref[p] == "C"][-64:]
    behind = [p for p in range(seam, seam + 100) if B.ref[p] == "C"][:5]
    B.add("ends", seam - 230, [(400, "M")], only=front)
    B.add("ends", seam - 220, [(380, "M")])
    B.add("goes_on", 1_990, [(5, "M"), (seam - 5 - 1_995, "N"), (100, "M")])
    B.add("goes_on", seam - 230, [(400, "M")], only=front + behind)
    B.add("goes_on", seam - 220, [(380, "M")])
    B.add("no_events", 1_500, [(40, "S"), (300, "M")], only="clip")
    B.add("no_events", 1_510, [(300, "M")])
    # (b') under -i a foreign segment without one of the owner's events: the owner's calls all lie in the interval in front of the
    # consumer's (`zero_front`: the search for the segment's first event runs to the list's end) or in the one behind it (`zero_behind`:
    # the first event found lies at or past p_hi); the consumer lies inside one interval, so nothing merges
    B.add("zero_front", 900, [(500, "M")], only=[p for p in range(900, 1_000) if B.ref[p] == "C"])
    B.add("zero_front", 1_005, [(295, "M")])
    B.add("zero_behind", 1_900, [(500, "M")], only=[p for p in range(2_000, 2_100) if B.ref[p] == "C"])
    B.add("zero_behind", 1_905, [(85, "M")])
    # (c) owner events on p_hi - 1 and p_hi of the segment [3000, 4000) and on p_lo - 1 and p_lo of [4000, 5000): the same trick at the
    # seam at 4000, every record calling every C, 3999 and 4000 among them
    B.add("edges", 2_950, [(30, "M"), (3_995 - 2_980, "N"), (300, "M")])
    B.add("edges", 3_900, [(200, "M")])
    B.add("edges", 3_950, [(250, "M")])
    # (d) three segments: `three` owns [1000, 2000), sits in an `N` op when [2000, 3000) begins, where the second record starts and
    # owns, and owns [3000, 4000) again, where the second record has ended
    B.add("three", 1_700, [(250, "M"), (300, "N"), (900, "M")])
    B.add("three", 2_010, [(700, "M")])
    B.background(0, CONTIG_LEN - 10, depth=1)
    c = B.finish("batches", "bt", prefix)
    for n in BATCH_EVENTS:
        own, con = c.records[c.index("batch%03d" % n)], c.records[c.index("batch%03d" % n, 1)]
        assert len(call_positions(own)) == n and own[0] // INTERVAL == (own[0] + 420) // INTERVAL
        assert all(con[0] <= p < con[0] + 400 for p in call_positions(own))
    for nm, k, lo, hi in (("ends", 0, 64, 0), ("goes_on", 1, 64, 5), ("no_events", 0, 0, 0)):
        ps = call_positions(c.records[c.index(nm, k)])
        assert (sum(1 for p in ps if p < seam), sum(1 for p in ps if p >= seam)) == (lo, hi)
    assert mf.written_calls(c.records[c.index("no_events")])[0][0][2], "the owner without events lists calls"
    asked = owners(c, interval=INTERVAL)
    for nm, lo, hi in (("zero_front", 900, 1_000), ("zero_behind", 2_000, 2_100)):      # one foreign segment, [1000, 2000), of 0 events
        own, con = c.index(nm), c.index(nm, 1)
        ps = call_positions(c.records[own])
        assert len(ps) > 20 and all(lo <= p < hi for p in ps) and asked[con] == [(1000, own, True, asked[own][0][3])]
        assert 1_000 <= c.records[con][0] and c.records[con][0] + ref_span(c.records[con][2]) <= 2_000
    taker, owner, con = (c.index("goes_on", k) for k in range(3))
    assert [(s, o) for s, o, _, _ in asked[con]] == [(2000, owner), (3000, taker)]
    taker, owner, con = (c.index("edges", k) for k in range(3))
    assert [(s, o) for s, o, _, _ in asked[con]] == [(3000, owner), (4000, taker)]
    assert all({3_999, 4_000} <= call_positions(c.records[i]) for i in (taker, owner)) and {3_999, 4_000} <= set(states(c.records[con]))
    x, y = c.index("three"), c.index("three", 1)
    assert [(s, o) for s, o, _, _ in asked[x]] == [(1000, x), (2000, y), (3000, x)] and [(s, o) for s, o, _, _ in asked[y]] == [(2000, y)]
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
def long_cigar(n_ops):
    """n_ops ops: M runs of 2-4 bases between 1-base D / I (now and then a 3-base N), one M of 150; an even count begins on a soft clip"""
    ops = [(3, "S")] if n_ops % 2 == 0 else []
    first = len(ops)
    for k in range(n_ops - first):
        if k % 2 == 0:
            ops.append((150 if k == 2 * (n_ops // 3) else 2 + k % 3, "M"))
        else:
            ops.append((3, "N") if k % 20 == 9 else (1, "DI"[(k // 2) % 2]))
    assert len(ops) == n_ops and ops[-1][1] == "M"
    return ops


def cigar(prefix):
    """2. the CIGAR walk of mkp_dup_events: consumers of 255 / 256 / 257 / 513 ops (1-base D and I between short M runs, one op of 150
    bases, a few `N` ops); owner calls on a consumer's M base, inside its D, its N and in front of it where its soft clip would lie, on
    its ref_start - 1, ref_start, ref_end - 1 and ref_end; on odd and even query indexes and on the last base of SEQ."""
    B = Book(211, c_every=3)
    at, spans = 100, {}
    for n_ops in LONG_OP_COUNTS:
        ops = long_cigar(n_ops)
        span = ref_span(ops)
        for p in (at - 1, at, at + span - 1, at + span):
            B.ref[p] = "C"
        for rev in (False, True):
            nm = "ops%03d_%d" % (n_ops, rev)
            B.add(nm, at - 30, [(span + 60, "M")], "m", rev)
            B.add(nm, at, ops, "m", rev)
        spans[n_ops] = (at, span)
        at += span + 80
    assert at < CONTIG_LEN
    B.background(0, at, depth=1)
    c = B.finish("cigar", "cg", prefix)
    for n_ops in LONG_OP_COUNTS:
        own, con = c.records[c.index("ops%03d_0" % n_ops)], c.records[c.index("ops%03d_0" % n_ops, 1)]
        assert len(con[2]) == n_ops and max(n for n, op in con[2]) >= 128 and {"D", "I", "N"} <= {op for _, op in con[2]}
        calls, st = call_positions(own), states(con)
        s, e = con[0], con[0] + ref_span(con[2])
        assert {s - 1, s, e - 1, e} <= calls
        on = [st[p] for p in calls if p in st]
        assert "D" in on and "N" in on and any(q != "D" and q != "N" and q % 2 for q in on) and any(q != "D" and q != "N" and not q % 2 for q in on)
        assert st[e - 1] == len(con[3]) - 1                    # the last base of SEQ, under an owner call
        if con[2][0][1] == "S":
            assert any(s - con[2][0][0] <= p < s for p in calls)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
STRAND_LAYOUTS = ("m", "h_m", "dx_m", "neg_only", "m_dot")
QUIET = (300, 900)          # no reverse background read here


def bases_strands(prefix):
    """3. the base test and the strands: every pair of owner / consumer strands under owners tagged `C+m?`, `C+h?;C+m?`, `C+m?;G-m?`,
    `G-m?` and `C+m.`; the consumer 40 bases on and as long as the owner (its last 40 columns are past the owner's end), with a SNP and an
    `N` on owner calls; a reverse consumer of a forward owner carries on three owner calls the base that matches in read orientation."""
    B = Book(221)
    at, pairs = 310, []
    for orev, crev in ((False, True), (False, False), (True, False), (True, True)):
        for lay in STRAND_LAYOUTS:
            nm = "%s_%d%d" % (lay, orev, crev)
            own = B.add(nm, at, [(200, "M")], lay, orev)
            calls = sorted(p for p in call_positions(own) if at + 40 <= p < at + 200)
            assert len(calls) >= 8, (nm, len(calls))
            force = {calls[0]: {"A": "C", "C": "A", "G": "T", "T": "G"}[B.ref[calls[0]]], calls[1]: "N"}
            if orev != crev:            # the stored base whose read-orientation base is the owner's call base
                force.update({p: cm.COMP[B.ref[p]] for p in calls[2:5]})
            B.add(nm, at + 40, [(200, "M")], lay, crev, force=force)
            pairs.append((nm, orev, crev, calls))
            at += 270
    assert at < CONTIG_LEN
    B.background(0, QUIET[0] - 200, depth=1)
    B.background(QUIET[0] - 100, QUIET[1] + 100, depth=2, mean=200, reverse=False)
    B.background(QUIET[1] + 200, CONTIG_LEN - 10, depth=1)
    c = B.finish("bases_strands", "bs", prefix)
    assert {(o, k) for _, o, k, _ in pairs} == {(False, True), (False, False), (True, False), (True, True)}
    for nm, orev, crev, calls in pairs:
        own, con = c.records[c.index(nm)], c.records[c.index(nm, 1)]
        assert bool(own[1] & 16) == orev and bool(con[1] & 16) == crev and own[0] + 40 == con[0]
        assert con[3][calls[1] - con[0]] == "N" and con[3][calls[0] - con[0]] != c.ref[calls[0]]
    # a column whose only '-' records are consumers of '+' owners
    lonely = 0
    for p in range(*QUIET):
        minus = [i for i, rec in enumerate(c.records) if rec[1] & 16 and rec[0] <= p < rec[0] + ref_span(rec[2])]
        if minus and all(c.read_names.count(c.read_names[i]) == 2 and c.index(c.read_names[i], 1) == i
                         and not c.records[c.index(c.read_names[i])][1] & 16 for i in minus):
            lonely += 1
    assert lonely > 100, lonely
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# spans of --include-bed that cut the groups of `ownership`: inside `same_start`; beginning inside the `N` op of `in_n`'s first record (the
# second owns, as it does not without the BED); over the seam and the deletion of `first_del`; behind the first record of `abc` (the second
# owns where the first did); over the seam inside `four`; one end of `shard_cut`; a gap over `late_focus`; the spans over `first_del` and `abc` are of one strand
BED_SPANS = ((120, 300, "."), (1_100, 1_300, "."), (1_990, 2_100, "-"), (3_080, 3_300, "+"), (3_620, 4_100, "."), (5_200, 5_300, "."))


def ownership(prefix):
    """4. who is asked first: two records on one start (file order); a member inside its own `N` op when the interval begins; a member
    whose first column of the interval is a deletion (it owns); under --cpg a record that starts first and reaches a focus position
    later; three and four records of a name (A, B, C where B and C meet and A does not); groups over interval seams, a --region start,
    shard cuts and the spans of a BED (BED_SPANS).  Every record is tagged `C+m?` with ML bytes of its own, so who owns shows in the calls and no
    record meets owners of different codes."""
    B = Book(231, edits=[(2_108, "AAAAAAATTTTT"), (2_132, "CG")])
    B.add("same_start", 100, [(300, "M")], "m")
    B.add("same_start", 100, [(280, "M")], "m")
    B.add("in_n", 700, [(250, "M"), (200, "N"), (150, "M")], "m")              # the N op lies over the seam at 1000
    B.add("in_n", 1_005, [(300, "M")], "m")
    B.add("first_del", 1_800, [(195, "M"), (12, "D"), (150, "M")], "m")          # the D op lies over the seam at 2000
    B.add("first_del", 2_003, [(200, "M")], "m")
    B.add("late_focus", 2_110, [(5, "M"), (60, "N"), (200, "M")], "m")           # its first CpG lies behind the N op; the other's at 2132
    B.add("late_focus", 2_120, [(200, "M")], "m")
    B.add("abc", 2_500, [(150, "M")], "m")                                       # A: interval 2 only
    B.add("abc", 3_050, [(300, "M")], "m")                                      # B and C meet in interval 3
    B.add("abc", 3_100, [(300, "M")], "m")
    for k, (s, lay) in enumerate(((3_600, "m"), (3_650, "m"), (3_700, "m"), (3_990, "m"))):   # four, over the seam at 4000
        B.add("four", s, [(420 - 60 * k, "M")], lay, reverse=k % 2 == 1)
    B.add("region_cut", REGION[0] - 60, [(400, "M")], "m")                       # --region starts inside the first: the second owns nothing new
    B.add("region_cut", REGION[0] - 20, [(400, "M")], "m")
    B.add("shard_cut", 4_900, [(400, "M")], "m")                                 # over 5000: an interval seam and, with --shard-bp 2500, a shard's
    B.add("shard_cut", 4_950, [(400, "M")], "m")
    B.background(0, CONTIG_LEN - 10, depth=1)
    c = B.finish("ownership", "ow", prefix)
    c.bed_spans = prefix + "_spans.bed"
    with open(c.bed_spans, "w") as f:
        for a, b, strand in BED_SPANS:
            f.write("%s\t%d\t%d%s\n" % (c.contig, a, b, "" if strand == "." else "\tspan\t0\t" + strand))
    one, grid, cpg = owners(c), owners(c, interval=INTERVAL), owners(c, motif=("CG", 0))
    first = lambda nm, k=0: c.index(nm, k)
    assert c.records[first("same_start")][0] == c.records[first("same_start", 1)][0] and one[first("same_start", 1)][0][1] == first("same_start")
    assert [(s, o) for s, o, _, _ in grid[first("in_n")]] == [(0, first("in_n")), (1000, first("in_n", 1))]
    st = states(c.records[first("first_del")])
    assert st[2000] == "D" and [(s, o) for s, o, _, _ in grid[first("first_del", 1)]] == [(2000, first("first_del"))]
    assert one[first("late_focus", 1)][0][1] == first("late_focus") and cpg[first("late_focus")][0][1] == first("late_focus", 1)
    assert [grid[first("abc", k)][0][1] for k in range(3)] == [first("abc"), first("abc", 1), first("abc", 1)]
    assert one[first("abc", 2)][0][1] == first("abc")
    assert len({grid[first("four", k)][-1][1] for k in range(4)}) == 1 and len(grid[first("four")]) == 2
    spans = owners(c, bed=list(BED_SPANS))
    assert one[first("in_n", 1)][0][1] == first("in_n") and spans[first("in_n", 1)][0][1] == first("in_n", 1)
    assert one[first("abc", 1)][0][1] == first("abc") and spans[first("abc", 1)][0][1] == first("abc", 1) and first("abc") not in spans
    assert first("late_focus") not in spans and spans[first("shard_cut", 1)][0][1] == first("shard_cut")
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
EDGE = 50


def status(prefix):
    """5. the owner's status: an owner whose ML is too short, one whose delta list runs past the read, each with a good consumer; a good
    owner with a broken consumer; under --edge-filter 50 an owner too short to trim with a long consumer and the reverse, and an owner
    whose every call is filtered."""
    B = Book(241)
    B.add("short_ml", 100, [(300, "M")], spoil="short_ml")
    B.add("short_ml", 130, [(300, "M")])
    B.add("runaway", 600, [(300, "M")], spoil="runaway")
    B.add("runaway", 640, [(300, "M")], reverse=True)
    B.add("bad_consumer", 1_100, [(300, "M")])
    B.add("bad_consumer", 1_120, [(300, "M")], spoil="short_ml")
    B.add("short_owner", 1_600, [(EDGE - 10, "M")])
    B.add("short_owner", 1_610, [(300, "M")])
    B.add("short_consumer", 2_100, [(300, "M")])
    B.add("short_consumer", 2_200, [(EDGE, "M")])
    cs = [p for p in range(2_600, 2_600 + 120) if B.ref[p] == "C" and not 2_600 + EDGE <= p < 2_600 + 120 - EDGE]
    B.add("all_filtered", 2_600, [(120, "M")], only=cs)
    B.add("all_filtered", 2_610, [(300, "M")])
    B.background(0, 3_200, depth=2)
    c = B.finish("status", "st", prefix)
    ef = cm.EdgeFilter(EDGE, EDGE)
    plain, edged = owners(c), owners(c, edge_filter=ef)
    good = lambda asked, nm, k: asked[c.index(nm, k)][0][2]
    assert len(cs) >= 4 and call_positions(c.records[c.index("all_filtered")]) == set(cs)
    assert [good(plain, nm, 1) for nm in ("short_ml", "runaway", "bad_consumer", "short_owner", "short_consumer", "all_filtered")] == \
        [False, False, True, True, True, True]
    assert [good(edged, nm, 1) for nm in ("short_owner", "short_consumer", "all_filtered")] == [False, True, False]
    assert not ef.read_can_be_trimmed(len(c.records[c.index("short_owner")][3])) and not ef.read_can_be_trimmed(len(c.records[c.index("short_consumer", 1)][3]))
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
def partition(prefix):
    """6. one name in two HP keys inside one interval, in both file orders, and in one key."""
    B = Book(251)
    B.add("two_keys", 200, [(300, "M")], "m", key=1)
    B.add("two_keys", 240, [(300, "M")], "hm", key=2)
    B.add("two_keys_back", 800, [(300, "M")], "hm", key=2)
    B.add("two_keys_back", 850, [(300, "M")], "m", key=1)
    B.add("one_key", 1_400, [(300, "M")], "m", key=1)
    B.add("one_key", 1_450, [(300, "M")], "hm", key=1)
    B.add("no_key", 2_000, [(300, "M")], "m", key=None)
    B.add("no_key", 2_030, [(300, "M")], "hm", key=2)
    B.background(0, 2_600, depth=3, keys=(1, 2, None))
    c = B.finish("partition", "pt", prefix)
    assert [c.keys[c.index("two_keys", k)] for k in (0, 1)] == [1, 2] and [c.keys[c.index("two_keys_back", k)] for k in (0, 1)] == [2, 1]
    assert {c.keys[c.index("one_key", k)] for k in (0, 1)} == {1} and set(c.keys) == {1, 2, None}
    return c


BUILDERS = {"batches": batches, "cigar": cigar, "bases_strands": bases_strands, "ownership": ownership, "status": status,
            "partition": partition}


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. owners that disagree: every shape is a BAM of its own, since the device refuses the whole run.  (name: (records, flags));
# records: (name, start, CIGAR, layout, spoil)
MIXED_SHAPES = {
    # the shape of tests/test_gpu_dup_names.py::test_owners_that_disagree_are_refused: B is answered from A (5mC) in the first interval
    # and from itself (5hmC, 5mC) in the second
    "codes_differ": ([("x", 110, [(100, "M")], "m", None), ("x", 140, [(300, "M")], "hm", None)], ["-i", "150"]),
    "status_differs": ([("x", 110, [(100, "M")], "m", "short_ml"), ("x", 140, [(300, "M")], "m", None)], ["-i", "150"]),
    # the neighbours that are not mixed: the same tags; an owner change (A, then C itself) where status and codes agree; one interval
    "same_tags": ([("x", 110, [(100, "M")], "m", None), ("x", 140, [(300, "M")], "m", None)], ["-i", "150"]),
    "owner_changes": ([("x", 110, [(100, "M")], "hm", None), ("x", 140, [(120, "M")], "hm", None), ("x", 160, [(400, "M")], "hm", None)], ["-i", "150"]),
    "one_interval": ([("x", 110, [(100, "M")], "m", None), ("x", 140, [(300, "M")], "hm", None)], []),
    "both_bad": ([("x", 110, [(100, "M")], "m", "short_ml"), ("x", 140, [(300, "M")], "m", "runaway")], ["-i", "150"]),
}
MIXED = {"codes_differ": True, "status_differs": True, "same_tags": False, "owner_changes": False, "one_interval": False, "both_bad": False}


def mixed(shape, prefix):
    B = Book(261)
    for nm, start, cg, lay, spoil in MIXED_SHAPES[shape][0]:
        B.add(nm, start, cg, lay, spoil=spoil)
    B.background(0, 800, depth=3, mean=150)
    c = B.finish("mixed_" + shape, "mx", prefix)
    c.flags = ["--no-filtering"] + MIXED_SHAPES[shape][1]
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# the flag sets of the device / oracle / model comparison

def flag_sets(case):
    """The command lines (without --tile, the device's own knob) every BAM runs under."""
    ref = ["--ref", case.fa]
    thr, nof = ["--filter-threshold", str(THRESHOLD)], ["--no-filtering"]
    out = []
    for focus in ([], ["--cpg"] + ref, ["--include-bed", case.bed], ["--cpg", "--combine-strands"] + ref):
        out += [focus + nof, focus + thr, focus + thr + ["-i", str(INTERVAL)], focus + nof + ["--region", "%s:%d-%d" % (case.contig, REGION[0], REGION[1])]]
    if case.name == "ownership":
        out += [["--cpg"] + ref + thr + ["-i", str(INTERVAL), "--shard-bp", "2500"], nof + ["-i", str(INTERVAL), "--shard-bp", "2500"]]
        spans = ["--include-bed", case.bed_spans]        # a BED of several spans, some of one strand, that cut the groups
        out += [spans + thr, ["--cpg"] + ref + spans + nof, spans + nof + ["-i", str(INTERVAL)]]
    if case.name == "status":
        out += [f + ["--edge-filter", str(EDGE)] for f in (nof, ["--cpg"] + ref + thr, ["--include-bed", case.bed] + thr + ["-i", str(INTERVAL)])]
    return out


def model_rows(case, flags, walked):
    """(the rows tests/column_model.py gives under `flags` (per key for a case with partition keys), the run's numbers for FLOORS, the
    records the model reports as mixed).  walked: a dict that keeps the walks of this case from one flag set to the next."""
    kw, edge = mf.model_kwargs(case, flags)
    if "--include-bed" in flags:          # the spans of the file the flag set names
        kw["bed"] = []
        for ln in open(flags[flags.index("--include-bed") + 1]):
            c = ln.split()
            kw["bed"].append((int(c[1]), int(c[2]), c[5] if len(c) > 5 else "."))
    ef = cm.EdgeFilter(*edge) if edge else None
    keyed = any(k is not None for k in case.keys)
    report = cm.new_report()
    rows = cm.pileup(case.records, case.ref, edge_filter=ef, names=case.read_names, keys=case.keys if keyed else None, report=report,
                     walk_cache=walked.setdefault((kw["threshold"], ef), {}), **kw)
    n_rows = sum(len(v) for v in rows.values()) if keyed else len(rows)
    return rows, (n_rows, report["rows_touched"], report["kept"], report["dropped"]), cm.mixed_records(report)


# (rows, rows a record answered from another one counts in, calls such a record found, owner calls its own base did not match) per flag
# set, as tests/column_model.py gives them on the CPU; tests/test_column_model.py holds them equal to the model's
FLOORS = {
    "batches": [(3234, 1834, 1023, 0), (2303, 1302, 1023, 0), (2328, 1222, 1109, 0), (1950, 1079, 736, 0), (1078, 407, 232, 0), (769, 281, 232, 0), (770, 266, 256, 0), (614, 248, 170, 0), (3234, 1834, 1023, 0), (2303, 1302, 1023, 0), (2328, 1222, 1109, 0), (3234, 1834, 1023, 0), (815, 478, 232, 0), (631, 371, 232, 0), (644, 374, 256, 0), (456, 301, 170, 0)],
    "cigar": [(2541, 2157, 1737, 0), (1951, 1671, 1737, 0), (1951, 1671, 1737, 0), (1370, 1168, 996, 0), (996, 841, 622, 0), (793, 670, 622, 0), (793, 670, 622, 0), (536, 467, 376, 0), (2541, 2157, 1737, 0), (1951, 1671, 1737, 0), (1951, 1671, 1737, 0), (2541, 2157, 1737, 0), (593, 500, 622, 0), (556, 470, 622, 0), (556, 470, 622, 0), (296, 258, 376, 0)],
    "bases_strands": [(2977, 1220, 528, 522), (2354, 923, 528, 522), (2354, 923, 528, 522), (1559, 758, 299, 291), (1005, 405, 186, 181), (789, 299, 186, 181), (789, 299, 186, 181), (527, 249, 112, 102), (2977, 1220, 528, 522), (2354, 923, 528, 522), (2354, 923, 528, 522), (2977, 1220, 528, 522), (764, 532, 186, 181), (651, 452, 186, 181), (651, 452, 186, 181), (382, 284, 112, 102)],
    "ownership": [(2634, 1043, 477, 116), (1990, 844, 477, 116), (2048, 824, 543, 116), (1524, 682, 255, 116), (947, 411, 184, 41), (723, 334, 184, 41), (738, 324, 211, 39), (550, 287, 107, 41), (2634, 1043, 477, 116), (1990, 844, 477, 116), (2048, 824, 543, 116), (2634, 1043, 477, 116), (793, 411, 184, 41), (632, 337, 184, 41), (644, 320, 212, 41), (448, 269, 107, 41), (738, 324, 211, 39), (2694, 1017, 543, 116), (559, 464, 291, 116), (253, 216, 98, 41), (685, 570, 291, 116)],
    "status": [(1866, 378, 111, 0), (1479, 281, 111, 0), (1479, 281, 111, 0), (1049, 61, 40, 0), (581, 119, 34, 0), (434, 74, 34, 0), (434, 74, 34, 0), (324, 20, 13, 0), (1866, 378, 111, 0), (1479, 281, 111, 0), (1479, 281, 111, 0), (1866, 378, 111, 0), (426, 207, 34, 0), (352, 169, 34, 0), (352, 169, 34, 0), (228, 85, 13, 0), (1516, 305, 65, 0), (321, 57, 18, 0), (1149, 228, 65, 0)],
    "partition": [(3852, 434, 266, 0), (2759, 334, 266, 0), (2759, 334, 266, 0), (1808, 160, 138, 0), (1209, 148, 96, 0), (895, 110, 96, 0), (889, 110, 96, 0), (578, 60, 54, 0), (3852, 434, 266, 0), (2759, 334, 266, 0), (2759, 334, 266, 0), (3852, 434, 266, 0), (860, 153, 96, 0), (708, 124, 96, 0), (708, 124, 96, 0), (404, 60, 54, 0)],
}
