"""Directed duplex modBAMs for the `pileup-hemi` kernels: reads on the 64-entry rank windows of mkp_merge_duplex, '+' / '-' pairs whose
halves sit in different 64-lane batches of a read's merged event list or either side of a tile, interval, region or shard seam, CIGARs
on the 128-op window of the hemi tile walk and the 64-op window of the event decoders, reads on the 4096-base step of the SPARSE decoder,
and records whose tags fail over 1, 2 and 5 intervals.

Built on the writers of tests/bamfuzz.py and the Case / Layer of tests/cigar_edge_cases.py, whose builders stay as they are.  Every
read's SEQ comes from its own CIGAR walked over the reference (about 3 % mismatches, a few `N` bases); the ML bytes are the fixed
pattern over {250, 10, 140} on one code of a call (which one also comes from the pattern) and 2 on every other code, so with
--filter-threshold 0.7 every call is modified, canonical or filtered, far from the threshold and from ties.  Both alignment strands are
used throughout.  A read carries the tags of one base pair: `C+..;G-..` (the halves of a CG 0 / CCGG 0 / CCGG 1 pair) or `G+..;C-..`
(the halves of a CG 1 / GC 0 pair: with C/G tags those motifs give NoCall everywhere), so every directed shape is written for both.
"""
import random

import cigar_edge_cases as cases
from bamfuzz import revcomp
from cigar_edge_cases import Case, gapped_cigar, ml_pattern, ref_span

THRESHOLD = cases.THRESHOLD
TILE = cases.TILE
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

# name: (base of the own-strand group, codes of each tag of a group, decode class).  The class is what class_ids (mkp_plan.hpp) gives a
# read of that layout under pileup-hemi: 5 = two groups of one tag each, 6 = two groups of two tags over one rank list each (both decoded
# per group by a SPARSE wave and interleaved by mkp_merge_duplex), 4 = the general decoder (here: three tags per group, more than the
# duplex classifier takes).
LAYOUTS = {
    "m": ("C", ["m"], 5),
    "hm": ("C", ["hm"], 5),
    "chebi": ("C", ["21839"], 5),
    "h_m": ("C", ["h", "m"], 6),
    "c3": ("C", ["m", "21839", "h"], 4),
    "g_m": ("G", ["m"], 5),
    "g_h_m": ("G", ["h", "m"], 6),
    "g3": ("G", ["m", "21839", "h"], 4),
}
MERGE_CLASSES, GENERAL_CLASS = (5, 6), 4
C_LAYOUTS, G_LAYOUTS = ("m", "h_m", "c3", "hm", "chebi"), ("g_m", "g_h_m", "g3")
# every directed shape is written once per entry: for each base pair the two merge classes and the general decoder, on both strands
DIRECTED = (("m", False), ("h_m", True), ("c3", False), ("g_m", True), ("g_h_m", False), ("g3", True))

MOTIFS = (("CG", 0), ("CG", 1), ("CCGG", 0), ("CCGG", 1), ("GC", 0))   # partner offsets +1, -1, +3, +1, +1


def pair_base(motif):
    """the base pair whose tags give calls on both halves of the motif: the base of the '+' focus position"""
    return motif[0][motif[1]]


def make_ref(r, n):
    """random text with a CpG every 25 bases, a CCGG every 175 and a GC every 75"""
    s = cases.make_ref(r, n)
    for p in range(40, n - 4, 175):
        s[p:p + 4] = "CCGG"
    for p in range(65, n - 2, 75):
        s[p:p + 2] = "GC"
    return s


def make_read(r, ref, start, cigar, layout, reverse, seed, flag=0, force=None, keep=None, broken=None):
    """One duplex record (start, flag, cigar, seq, MM, ML).
    force: {reference position: base} written into SEQ where the read has a base there (a SNP, an `N`, or the reference's own base where
    a directed pair must not be lost to a random mismatch).
    keep: f(events) -> the events to list, of events = [(reference position or None, 'A' | 'B', rank among the group's bases, the base
    as stored in SEQ)] in as-sequenced order; default: every base of both groups.
    broken: None | 'short_ml' | 'overrun_a' | 'overrun_b' | 'empty' (no call listed by either group)."""
    start, flag, cigar, seq, _, _ = cases.make_read(r, ref, start, cigar, "m", reverse, seed, flag)
    where, p, q = {}, start, 0          # index into SEQ -> reference position
    for n, op in cigar:
        if op in "M=X":
            for k in range(n):
                where[q + k] = p + k
        if op in "MDN=X":
            p += n
        if op in "MIS=X":
            q += n
    if force:
        seq = list(seq)
        for q, p in where.items():
            if p in force:
                seq[q] = force[p]
        seq = "".join(seq)
    fwd = revcomp(seq) if reverse else seq
    L = len(seq)
    base, tags, _ = LAYOUTS[layout]
    events = []
    for g, b in (("A", base), ("B", COMP[base])):
        events += [(i, g, k) for k, i in enumerate(i for i, c in enumerate(fwd) if c == b)]
    events.sort()
    events = [(where.get(L - 1 - i if reverse else i), g, k, seq[L - 1 - i if reverse else i]) for i, g, k in events]
    listed = events if keep is None else keep(events)
    if broken == "empty":
        listed = []
    mm, ml = "", []
    for g, head in (("A", base + "+"), ("B", COMP[base] + "-")):
        ranks = sorted(e[2] for e in listed if e[1] == g)
        deltas, last = [], -1
        for k in ranks:
            deltas.append(k - last - 1); last = k
        if broken == "overrun_" + g.lower():
            deltas.append(L + 5)
        lst = "".join(",%d" % d for d in deltas)
        n_codes = sum(1 if t.isdigit() else len(t) for t in tags)
        pat = ml_pattern(seed * 2 + (g == "B"), len(deltas))
        hot = [(i * 7 + seed + (g == "B")) % n_codes for i in range(len(deltas))]     # the code of each call that carries the pattern's byte
        j0 = 0
        for t in tags:
            k_codes = 1 if t.isdigit() else len(t)
            mm += "%s%s?%s;" % (head, t, lst)
            for i in range(len(deltas)):
                ml += [pat[i] if hot[i] == j0 + j else 2 for j in range(k_codes)]
            j0 += k_codes
    if broken == "short_ml":
        ml = ml[:-2]
    return start, flag | (16 if reverse else 0), list(cigar), seq, mm, ml


class Layer(cases.Layer):
    """cigar_edge_cases.Layer with duplex reads; successive directed reads overlap by three quarters"""

    def add(self, cigar, layout="m", reverse=None, start=None, flag=0, name=None, **kw):
        k = len(self.records)
        if start is None:
            start = self.at
            self.at += ref_span(cigar) // 4 + 17
        rev = (k % 2 == 1) if reverse is None else reverse
        self.records.append(make_read(self.r, self.ref, start, cigar, layout, rev, 1000 + k, flag, **kw))
        self.names.append(name or "e%05d" % k)
        self.layouts.append(layout)
        return start

    def background(self, lo, hi, depth=8, mean=400, layouts=tuple(LAYOUTS)):
        cases.Layer.background(self, lo, hi, depth, mean, layouts)

    def deep_column(self, pos, depth=300):
        """one column under about `depth` short reads"""
        for k in range(depth):
            n = self.r.randrange(40, 90)
            self.add([(n, "M")], ("m", "g_m", "h_m")[k % 3], k % 2 == 1, pos - self.r.randrange(2, n - 2), name="deep%04d" % k)

    def finish(self, lo, hi):
        self.background(lo, hi)
        self.deep_column(first_hit(self.ref, "CG", (lo + hi) // 2))
        self.flagged_copies()


def first_hit(ref, text, at):
    """the first position >= at where `text` lies in the reference"""
    n = len(text)
    while "".join(ref[at:at + n]) != text:
        at += 1
    return at


def keep_true_bases(ref, ps):
    """force argument that keeps the reference's own base at the positions `ps`"""
    return {p: ref[p] for p in ps if 0 <= p < len(ref)}


# ---------------------------------------------------------------------------------------------------------------------------------
MERGE_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 193)
MERGE_PAIRS = sorted({(v, v) for v in MERGE_SIZES} | {(v, 64) for v in MERGE_SIZES} | {(64, v) for v in MERGE_SIZES}
                     | {(v, 129) for v in MERGE_SIZES} | {(129, v) for v in MERGE_SIZES} | {(1, 193), (193, 1)})
SKEWED = ((129, 129), (193, 65), (65, 193))
MERGE_LAYOUTS = (("m", False), ("h_m", True), ("g_m", False), ("hm", True), ("g_h_m", False), ("chebi", True))


def _paired(events):
    """indexes of the events that are one half of an adjacent A-B or B-A pair on the reference (a CpG's C and G, a GpC's G and C)"""
    at = {e[0]: i for i, e in enumerate(events) if e[0] is not None}
    return {i for p, i in at.items() for d in (-1, 1) if p + d in at and events[at[p + d]][1] != events[i][1]}


def keep_counts(n_a, n_b):
    """list exactly n_a events of the first group and n_b of the second, halves of adjacent pairs first"""
    def keep(events):
        paired, out = _paired(events), []
        for g, n in (("A", n_a), ("B", n_b)):
            mine = [i for i, e in enumerate(events) if e[1] == g and e[0] is not None]
            assert len(mine) >= n, "the read is too short for %d events" % n
            out += sorted(mine, key=lambda i: (i not in paired, i))[:n]
        return [events[i] for i in out]
    return keep


def keep_skewed(n_a, n_b, a_first):
    """every listed event of one group lies before (as sequenced) every listed event of the other; the two that meet are the halves of
    one adjacent pair where the read has one there"""
    def keep(events):
        order = ("A", "B") if a_first else ("B", "A")
        n = dict(A=n_a, B=n_b)
        paired = _paired(events)
        first = [i for i, e in enumerate(events) if e[1] == order[0] and e[0] is not None]
        cut = first[n[order[0]] - 1]
        for j in range(n[order[0]] - 1, len(first)):      # end the first block on a paired event if one is near
            if first[j] in paired and first[j] + 1 < len(events) and events[first[j] + 1][1] == order[1]:
                cut = first[j]
                break
        head = [i for i in first if i <= cut][-n[order[0]]:]
        tail = [i for i, e in enumerate(events) if e[1] == order[1] and e[0] is not None and i > cut][:n[order[1]]]
        assert len(head) == n[order[0]] and len(tail) == n[order[1]], "the read is too short"
        return [events[i] for i in head + tail]
    return keep


def keep_one_strand_per_pair(events):
    """at every adjacent pair only one half is listed; everything else is listed"""
    paired = _paired(events)
    return [e for i, e in enumerate(events) if i not in paired or e[1] == "A"]


def merge_windows(prefix):
    """1. mkp_merge_duplex: per-group event counts on the edges of the 64-entry rank windows, skewed reads whose ranks jump whole
    windows, groups that list nothing, reads with one strand called at every pair.  Plain `M` reads: every listed call is an event."""
    r = random.Random(61)
    ref = make_ref(r, 100_000)
    L = Layer(62, ref)
    k = 0
    for n_a, n_b in MERGE_PAIRS:
        for j in range(2):
            layout, rev = MERGE_LAYOUTS[(k + j) % len(MERGE_LAYOUTS)]
            L.add([(1500, "M")], layout, rev, keep=keep_counts(n_a, n_b), name="mw%05d" % len(L.records))
        k += 1
    for n_a, n_b in SKEWED:
        for a_first in (True, False):
            for layout, rev in (("m", False), ("g_m", True), ("h_m", True), ("g_h_m", False)):
                L.add([(2600, "M")], layout, rev, keep=keep_skewed(n_a, n_b, a_first), name="sk%05d" % len(L.records))
    for layout, rev in DIRECTED:
        L.add([(700, "M")], layout, rev, keep=keep_one_strand_per_pair, name="one%05d" % len(L.records))
        L.add([(300, "M")], layout, rev, broken="empty", name="none%05d" % len(L.records))
    L.finish(0, L.at + 2700)
    assert L.at + 2700 < len(ref)
    return Case("merge_windows", "merge", "".join(ref), L, prefix)


# ---------------------------------------------------------------------------------------------------------------------------------
PARTNER_INDEXES = (63, 64, 127, 128)
# seams of the partner_edges BAM per motif text: --tile 256, -i 500, --shard-bp 3000 and the end of --region pe:1000-5000
SEAMS = {"CG": dict(tile=1024, interval=1500, shard=3000, region_end=5000), "CCGG": dict(tile=1280, interval=2000, shard=6000),
         "GC": dict(tile=1792, interval=2500, shard=9000)}
REGION = (1000, 5000)
BED_SPANS = ((900, 1600), (1600, 2100), (2900, 3100), (5990, 6400), (8000, 9001), (12000, 30000))


def keep_plus_half_at(index, motif, ref):
    """drop the earliest events until the '+' half of some complete pair of `motif` has exactly `index` events before it on the
    reference; the pair is the first one far enough into the read"""
    text, off = motif
    d = len(text) - 1 - 2 * off

    def keep(events):
        on_ref = sorted((e[0], i) for i, e in enumerate(events) if e[0] is not None)
        true = {p for p, i in on_ref if events[i][3] == ref[p]}            # events on a base that matches the reference
        for rank, (p, i) in enumerate(on_ref):
            lo = p - off
            # (a partner before the '+' half, d < 0, is the event just before it: it stays listed for every index above 0)
            if rank >= index and lo >= 0 and "".join(ref[lo:lo + len(text)]) == text and p in true and p + d in true:
                drop = {j for _, j in on_ref[:rank - index]}
                assert len(on_ref[:rank]) - len(drop) == index
                return [e for j, e in enumerate(events) if j not in drop]
        raise AssertionError("no pair of %s far enough into the read" % (motif,))
    return keep


def partner_edges(prefix):
    """2. the partner search of the hemi tile kernel: pairs whose '+' half has index 63 / 64 / 127 / 128 in the read's merged list, per
    motif; pairs either side of tile, interval, region and shard seams; every way a partner can be missing."""
    r = random.Random(71)
    ref = make_ref(r, 60_000)
    ref[0], ref[1] = "G", "C"                       # a G at contig position 0 (CG 1: the partner position would be -1)
    for text, seams in SEAMS.items():
        for s in seams.values():
            a = s - len(text) // 2
            ref[a:a + len(text)] = text                 # the motif's two halves lie either side of the seam
    sites = [p for p in range(12_007, 30_000, 25)]  # CpGs of make_ref, away from the seams
    for p in sites:
        assert ref[p] == "C" and ref[p + 1] == "G"
    L = Layer(72, ref)
    # (a) '+' halves on the lane-batch edges of the merged list
    for motif in MOTIFS:
        layouts = [x for x in DIRECTED if LAYOUTS[x[0]][0] == pair_base(motif)]
        for index in PARTNER_INDEXES:
            for layout, rev in layouts:
                L.add([(1300, "M")], layout, rev, keep=keep_plus_half_at(index, motif, ref), name="pe_%s%d_%d_%05d" % (motif[0], motif[1], index, len(L.records)))
                L.add([(1300, "M")], layout, not rev, keep=keep_plus_half_at(index, motif, ref), name="pe_%s%d_%d_%05d" % (motif[0], motif[1], index, len(L.records)))
    # (b) reads that begin, end and gap around the seam motifs
    for text, seams in SEAMS.items():
        for s in seams.values():
            a = s - len(text) // 2
            true = keep_true_bases(ref, range(a, a + len(text)))
            for layout, rev in DIRECTED:
                L.add([(90, "M"), (2, "D"), (120, "M")], layout, rev, s - 100, force=true, name="seam%05d" % len(L.records))
                L.add([(150, "M")], layout, not rev, s - 149, name="seam%05d" % len(L.records))        # ends on the last base before the seam
                L.add([(150, "M")], layout, rev, s, name="seam%05d" % len(L.records))                  # begins on the seam
    # (c) missing partners, each on a CpG of its own: p = the C, p + 1 = the G
    site = iter(sites[20::12])
    shapes = [
        ("ends_on_c", lambda p: dict(cigar=[(80, "M")], start=p - 79)),
        ("begins_on_g", lambda p: dict(cigar=[(80, "M")], start=p + 1)),
        ("g_clipped", lambda p: dict(cigar=[(80, "M"), (6, "S")], start=p - 79)),
        ("c_clipped", lambda p: dict(cigar=[(6, "S"), (80, "M")], start=p + 1)),
        ("d_on_g", lambda p: dict(cigar=[(60, "M"), (1, "D"), (40, "M")], start=p - 59)),
        ("d_on_c", lambda p: dict(cigar=[(60, "M"), (1, "D"), (40, "M")], start=p - 60)),
        ("n_on_g", lambda p: dict(cigar=[(60, "M"), (1, "N"), (40, "M")], start=p - 59)),
        ("n_on_c", lambda p: dict(cigar=[(60, "M"), (1, "N"), (40, "M")], start=p - 60)),
        ("d_on_both", lambda p: dict(cigar=[(60, "M"), (2, "D"), (40, "M")], start=p - 60)),
        ("i_between", lambda p: dict(cigar=[(60, "M"), (3, "I"), (40, "M")], start=p - 59)),
        ("snp_on_c", lambda p: dict(cigar=[(100, "M")], start=p - 50, force={p: "T", p + 1: "G"})),
        ("snp_c_to_g", lambda p: dict(cigar=[(100, "M")], start=p - 50, force={p: "G", p + 1: "G"})),
        ("snp_on_g", lambda p: dict(cigar=[(100, "M")], start=p - 50, force={p: "C", p + 1: "A"})),
        ("n_base_on_c", lambda p: dict(cigar=[(100, "M")], start=p - 50, force={p: "N", p + 1: "G"})),
        ("n_base_on_g", lambda p: dict(cigar=[(100, "M")], start=p - 50, force={p: "C", p + 1: "N"})),
    ]
    for what, shape in shapes:
        p = next(site)
        for layout, rev in DIRECTED:
            kw = shape(p)
            kw.setdefault("force", keep_true_bases(ref, (p, p + 1)))
            L.add(kw.pop("cigar"), layout, rev, name="%s_%05d" % (what, len(L.records)), **kw)
    for layout, rev in DIRECTED:
        L.add([(120, "M")], layout, rev, 0, force=keep_true_bases(ref, (0, 1)), name="at0_%05d" % len(L.records))
    top = max(L.at, 31_000)
    L.finish(0, top)
    c = Case("partner_edges", "pe", "".join(ref), L, prefix, seams={k: dict(v) for k, v in SEAMS.items()})
    c.spans_bed = prefix + "_spans.bed"
    with open(c.spans_bed, "w") as f:
        for a, b in BED_SPANS:
            f.write("%s\t%d\t%d\n" % (c.contig, a, b))
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
CIGAR_OP_COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
CIGAR_EDGE_INDEXES = ([63, 127, 255], [64, 128, 256])     # the last op of a 64-op / 128-op window, and the first of the next


def cigar_windows(prefix):
    """3. op counts on the edges of the hemi tile walk's 128-op window (two ops per lane) and the event decoders' 64-op window; D / I / N / P
    on the last op of a window and the first of the next, a CpG on the match run on each side."""
    r = random.Random(81)
    ref = make_ref(r, 90_000)
    L = Layer(82, ref)
    plan = []
    for n in CIGAR_OP_COUNTS:
        ops = gapped_cigar(L.r, n)
        for layout, rev in DIRECTED:
            plan.append((ops, layout, rev, None))
    for op in "DINP":
        for idxs, n_ops in zip(CIGAR_EDGE_INDEXES, (515, 516)):
            ops = gapped_cigar(L.r, n_ops, {i: (40 if op == "N" else 3, op) for i in idxs}, lo=2)
            for layout, rev in DIRECTED:
                plan.append((ops, layout, rev, idxs))
    # lay the reads out, put a CpG on the match run before and after every edge op, then write the reads over the finished reference
    at, placed, true = 50, [], {}
    for ops, layout, rev, idxs in plan:
        placed.append((ops, layout, rev, at, idxs))
        at += ref_span(ops) // 4 + 17
    for ops, layout, rev, start, idxs in placed:
        p = start
        for i, (n, op) in enumerate(ops):
            if idxs and (i + 1 in idxs or i - 1 in idxs) and op in "M=" and n >= 2:
                a = p if i - 1 in idxs else p + n - 2
                ref[a], ref[a + 1] = "C", "G"
            if op in "MDN=X":
                p += n
    for ops, layout, rev, start, idxs in placed:
        force = {}
        if idxs:
            p = start
            for i, (n, op) in enumerate(ops):
                if (i + 1 in idxs or i - 1 in idxs) and op in "M=":
                    force.update(keep_true_bases(ref, range(p, p + n)))
                if op in "MDN=X":
                    p += n
        L.add(ops, layout, rev, start, force=force, name="cw%05d" % len(L.records))
    L.at = at
    L.finish(0, at + 3000)
    assert at + 3000 < len(ref)
    return Case("cigar_windows", "cw", "".join(ref), L, prefix)


# ---------------------------------------------------------------------------------------------------------------------------------
SPARSE_LENGTHS = (4095, 4096, 4097, 8193)
SPARSE_PAIRS = (4095, 8191)      # stored positions of the C of a called C/G pair (the G one further)


def sparse_steps(prefix):
    """4. reads of 4095 / 4096 / 4097 / 8193 bases: the SPARSE decoder's 4096-base step; a called pair at stored positions 4095 / 4096
    and 8191 / 8192 on forward and reverse reads (a reverse read consumes its rank list from the end)."""
    r = random.Random(91)
    ref = make_ref(r, 100_000)
    L = Layer(92, ref)
    placed, at = [], 50
    for n in SPARSE_LENGTHS:
        for layout, rev in DIRECTED:
            for flip in (False, True):
                placed.append((n, layout, rev != flip, at))
                at += n // 4 + 31
    for n, layout, rev, start in placed:
        for q in SPARSE_PAIRS:
            if q + 1 < n:
                ref[start + q:start + q + 2] = "CG"
    for n, layout, rev, start in placed:
        true = keep_true_bases(ref, [start + q + d for q in SPARSE_PAIRS for d in (0, 1) if q + 1 < n])
        L.add([(n, "M")], layout, rev, start, force=true, name="sp%05d" % len(L.records))
    L.at = at
    L.finish(0, at + 8200)
    assert at + 8200 < len(ref)
    return Case("sparse_steps", "sp", "".join(ref), L, prefix)


# ---------------------------------------------------------------------------------------------------------------------------------
FAILED_INTERVAL = 500
FAILURES = ("short_ml", "overrun_a", "overrun_b", "empty")
FAILED_CROSSINGS = (1, 2, 5)


def failed_records(prefix):
    """5. records whose tags fail (an ML of the wrong length, a delta list past the read in either group, nothing listed) over 1, 2 and 5
    intervals of 500, starting on an interval's first base and in its middle; the first CpG of an interval under a deletion, a ref-skip
    and an `N` base; all among good reads over the same columns."""
    r = random.Random(101)
    ref = make_ref(r, 40_000)
    L = Layer(102, ref)
    at = 2_000
    for broken in FAILURES:
        for layout, rev in DIRECTED:
            for start_off, n in ((40, 300), (0, 500), (300, 450), (250, 2_200), (0, 2_500)):   # 1, 1, 2, 5, 5 intervals
                L.add([(n, "M")], layout, rev, at + start_off, broken=broken, name="bad_%s_%05d" % (broken, len(L.records)))
            at += 1_000
    # a five-interval record whose first CpG of the 2nd, 3rd and 4th interval lies under a D, an N, an `N` base
    for broken in FAILURES:
        for layout, rev in DIRECTED[:4]:
            start = at + 250
            c = [first_hit(ref, "CG", at + 500 * k) for k in (1, 2, 3)]
            ops = [(c[0] - start, "M"), (1, "D"), (c[1] - c[0] - 1, "M"), (3, "N"), (c[2] - c[1] - 3, "M"), (start + 2_200 - c[2], "M")]
            assert ref_span(ops) == 2_200
            L.add(ops, layout, rev, start, broken=broken, force={c[2]: "N"}, name="bad_gap_%s_%05d" % (broken, len(L.records)))
            at += 500
    L.at = at
    L.finish(1_500, at + 3_000)
    assert at + 3_000 < len(ref)
    return Case("failed_records", "fr", "".join(ref), L, prefix)


BUILDERS = {"merge_windows": merge_windows, "partner_edges": partner_edges, "cigar_windows": cigar_windows, "sparse_steps": sparse_steps,
            "failed_records": failed_records}


# ---------------------------------------------------------------------------------------------------------------------------------
# the flag sets of the device / oracle / model comparison

def flag_sets(case):
    """The pileup-hemi command lines (without -o, and without --tile, the device's own knob) every BAM runs under."""
    thr, nof = ["--filter-threshold", str(THRESHOLD)], ["--no-filtering"]
    sets = [["--cpg"] + nof, ["--cpg"] + thr, ["--motif", "CG", "1"] + nof, ["--motif", "CCGG", "0"] + thr, ["--motif", "GC", "0"] + nof,
            ["--cpg", "--combine-mods"] + nof]
    if case.name == "failed_records":
        sets += [["--cpg", "-i", str(FAILED_INTERVAL)] + nof, ["--motif", "CG", "1", "-i", str(FAILED_INTERVAL)] + thr]
    if case.name == "partner_edges":
        region = ["--region", "%s:%d-%d" % (case.contig, REGION[0], REGION[1])]
        sets += [["--cpg", "-i", "500"] + nof, ["--motif", "CCGG", "0", "-i", "500"] + thr, ["--motif", "GC", "0", "-i", "500"] + nof,
                 ["--motif", "CG", "1", "-i", "500"] + nof, ["--cpg"] + region + nof, ["--motif", "CG", "1"] + region + thr,
                 ["--cpg", "--include-bed", case.spans_bed, "-i", "500"] + nof,
                 ["--cpg", "-i", "500", "--shard-bp", "3000"] + thr, ["--motif", "CCGG", "0", "-i", "500", "--shard-bp", "3000"] + nof,
                 ["--motif", "GC", "0", "-i", "500", "--shard-bp", "3000"] + nof]
    return [s + ["-r", case.fa] for s in sets]


def oracle_flags(flags):
    return cases.oracle_flags(flags)


def model_kwargs(case, flags):
    kw, k = dict(threshold=None), 0
    while k < len(flags):
        f = flags[k]
        if f == "--filter-threshold":
            kw["threshold"] = float(flags[k + 1]); k += 1
        elif f == "-i":
            kw["interval"] = int(flags[k + 1]); k += 1
        elif f == "--cpg":
            kw["motif"] = ("CG", 0)
        elif f == "--motif":
            kw["motif"] = (flags[k + 1], int(flags[k + 2])); k += 2
        elif f == "--combine-mods":
            kw["combine_mods"] = True
        elif f == "--include-bed":
            kw["bed"] = [(a, b, ".") for a, b in BED_SPANS]; k += 1
        elif f == "--region":
            a, b = flags[k + 1].split(":")[1].split("-")
            kw["region"] = (int(a), int(b)); k += 1
        elif f in ("-r", "--shard-bp", "--tile"):
            k += 1
        else:
            assert f == "--no-filtering", f
        k += 1
    return kw


# (rows, rows with n_delete > 0, rows with n_nocall > 0, rows whose pattern is not `-,-`, columns with two or more patterns) per flag set:
# what tests/hemi_model.py gives on the CPU, less a tenth.  tests/test_hemi_model.py holds the model to them (and them to the model), so a
# later edit to a builder cannot silently empty a case.  Every flag set gives more than 100 rows; failed_records more than FAILED_MIN_ROWS.
FAILED_MIN_ROWS = 400
FLOORS = {
    "cigar_windows": [(17010, 8934, 16796, 15278, 3748), (8247, 4356, 8140, 6516, 2595), (12688, 6618, 12681, 11279, 3442), (667, 384, 664, 530, 208), (10282, 5330, 10280, 9117, 2806), (10800, 5713, 10669, 9068, 3627)],
    "failed_records": [(12263, 346, 12066, 10987, 3011), (5877, 164, 5777, 4600, 1835), (8264, 210, 8202, 7335, 2521), (514, 20, 510, 402, 151), (7165, 217, 7084, 6362, 2191), (8306, 240, 8152, 7029, 2862), (12263, 346, 12068, 10987, 3011), (3957, 95, 3932, 3027, 1124)],
    "merge_windows": [(19609, 522, 19589, 17599, 4542), (9473, 244, 9464, 7463, 2943), (11952, 337, 11943, 10622, 3472), (823, 13, 823, 645, 262), (10465, 308, 10455, 9293, 3012), (12785, 303, 12770, 10775, 4338)],
    "partner_edges": [(19856, 522, 19581, 17796, 3686), (10076, 270, 9945, 8016, 2921), (13889, 348, 13671, 12437, 3411), (909, 32, 891, 727, 263), (11736, 315, 11555, 10466, 2876), (11482, 289, 11331, 9422, 3598), (19856, 522, 19581, 17796, 3686), (909, 32, 891, 727, 263), (11736, 315, 11555, 10466, 2876), (13889, 348, 13671, 12437, 3411), (2523, 31, 2511, 2272, 369), (690, 4, 690, 543, 202), (10908, 322, 10692, 9805, 1886), (10076, 270, 9945, 8016, 2921), (1791, 72, 1752, 1608, 322), (11736, 315, 11555, 10466, 2876)],
    "sparse_steps": [(31237, 785, 30719, 27988, 6367), (15398, 392, 15143, 12149, 4671), (23338, 584, 23178, 20779, 5836), (1441, 34, 1424, 1142, 446), (19528, 429, 19396, 17397, 4879), (19105, 470, 18782, 15856, 6202)],
}
