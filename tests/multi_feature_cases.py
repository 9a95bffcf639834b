"""Directed modBAMs for the reads the fused slot decoder never takes: several primary bases in one read, tags on the read's '-' strand
(two features on one column), `N`-base tags, and any read once an edge filter is set.  They reach the kernels through the general event
decoder (mkp_decode_reads, decode class 4) or, where a read's tags form two explicit groups on different bases (`C+m?;G-m?`,
`C+m?;A+a?`, `C+h?;C+m?;G-h?;G-m?`, `C+h?;C+m?;A+a?`: decode classes 5 / 6, which `pileup` assigns as `pileup-hemi` does), through one SPARSE decode per group and
mkp_merge_duplex; then through mkp_cover_reads (which merges a read's position-sorted events into its slot stream 64 at a
time and puts a column's second feature on an overflow list), the overflow loops of mkp_pileup_stream and the event path of
mkp_pileup_tiles; the edge filter has one copy of its predicate in each of the three event decoders.

Built on the writers of tests/bamfuzz.py and the Case / Layer of tests/cigar_edge_cases.py, whose builders stay as they are.  A read's
SEQ comes from its own CIGAR walked over the reference (about 3 % mismatches, a few `N` bases; the reads with a planned event list carry
the reference's own bases).  Per (read strand, base) group one code of a call carries a byte of the pattern {250, 10, 140} and every other
code 2, so with --filter-threshold 0.7 every call is modified, canonical or filtered, far from the threshold and from ties.  Every code
belongs to one primary base (m, h, f, c, 21839: C; a: A; g: G; t: T), so rows of two primary bases on one column never share a name; the
`N` tag's code b is listed only on bases that match the reference, for the same reason.

Every BAM also holds plain `C+m?` / `C+h?;C+m?` reads (decode classes 0 / 1) over the same columns, so fused and covered reads share
tiles; every directed shape is on a forward and on a reverse record; contigs are 40 kb, reads at most 8 193 bases.
"""
import random

import cigar_edge_cases as cases
from bamfuzz import revcomp
from cigar_edge_cases import Case, ref_span

THRESHOLD = cases.THRESHOLD
TILE = cases.TILE
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CONTIG_LEN = 40_000
MAX_READ = 8_193

# name: the tags of a read, (fundamental base, strand, codes, mode) each
LAYOUTS = {
    "m": [("C", "+", ["m"], "?")],
    "h_m": [("C", "+", ["h"], "?"), ("C", "+", ["m"], "?")],
    "hm": [("C", "+", ["h", "m"], "?")],
    "m_dot": [("C", "+", ["m"], ".")],
    "h_m_dot": [("C", "+", ["h"], "."), ("C", "+", ["m"], ".")],
    "chebi": [("C", "+", ["21839"], "?")],
    "c4": [("C", "+", ["h", "m", "f", "c"], "?")],                                             # four codes in one tag
    "c4tags": [("C", "+", ["h"], "?"), ("C", "+", ["m"], "?"), ("C", "+", ["f"], "?"), ("C", "+", ["c"], "?")],   # four tags on one (strand, base)
    "c_a": [("C", "+", ["m"], "?"), ("A", "+", ["a"], "?")],
    "h_m_a": [("C", "+", ["h"], "?"), ("C", "+", ["m"], "?"), ("A", "+", ["a"], "?")],
    "acgt": [("A", "+", ["a"], "?"), ("C", "+", ["m"], "?"), ("G", "+", ["g"], "?"), ("T", "+", ["t"], "?")],
    "neg_only": [("G", "-", ["m"], "?")],                                                      # the negative feature alone
    "dx_m": [("C", "+", ["m"], "?"), ("G", "-", ["m"], "?")],                                  # duplex, one tag per group
    "dx_h_m": [("C", "+", ["h"], "?"), ("C", "+", ["m"], "?"), ("G", "-", ["h"], "?"), ("G", "-", ["m"], "?")],
    "dup_c": [("C", "+", ["m"], "?"), ("C", "-", ["g"], "?")],                                 # the same base on '+' and '-': two features per column
    "dup8": [("A", "+", ["a"], "?"), ("C", "+", ["m"], "?"), ("G", "+", ["g"], "?"), ("T", "+", ["t"], "?"),
             ("A", "-", ["t"], "?"), ("C", "-", ["g"], "?"), ("G", "-", ["m"], "?"), ("T", "-", ["a"], "?")],   # eight tags; any base, both strands
    "n_b": [("N", "+", ["b"], "?")],
    "n_b_m": [("N", "+", ["b"], "?"), ("C", "+", ["m"], "?")],
    "dx_dot": [("C", "+", ["m"], "."), ("G", "-", ["m"], ".")],
}
PLAIN = ("m", "h_m")


def decode_class(tags, rank_lists):
    """The decode class class_ids (mkp_plan.hpp) gives a good read of these tags when a shard is made resident, for `pileup` and for
    `pileup-hemi` alike (only the threshold sampler classifies without the duplex classes); restated from its rules and those of the
    layout tables (mkp_pack.hpp).  FAST: every tag on one (strand, base) that is not `N`, no code listed twice; with at most two tags it
    is class 0 / 1 (one / two tags) when every tag is explicit and two tags share one rank list, else class 2 / 3.  Duplex: a leading
    run of at most two tags on one (strand, base) and at most two more on one other, of a different base, no code twice inside a group;
    every tag explicit and the tags of a group sharing one rank list give class 5 (one tag per group) or 6: each group is decoded by a
    SPARSE wave and mkp_merge_duplex interleaves the two event lists.  Everything else is class 4, the general decoder."""
    if not tags:
        return 4
    groups = [(fb, s) for fb, s, _, _ in tags]
    explicit = all(mode == "?" for _, _, _, mode in tags)
    codes = [c for _, _, cs, _ in tags for c in cs]
    if all(g == groups[0] for g in groups) and groups[0][0] != "N" and len(set(codes)) == len(codes):
        if len(tags) <= 2:
            sparse = explicit and (len(tags) == 1 or rank_lists[0] == rank_lists[1])
            return (0 if sparse else 2) + len(tags) - 1
        return 4
    if 2 <= len(tags) <= 4:
        n_a = 1
        while n_a < len(tags) and groups[n_a] == groups[0]:
            n_a += 1
        rest = groups[n_a:]
        ok = bool(rest) and n_a <= 2 and len(rest) <= 2 and "N" not in (groups[0][0], rest[0][0]) and rest[0][0] != groups[0][0] \
            and all(g == rest[0] for g in rest)
        for part in (tags[:n_a], tags[n_a:]):
            cs = [c for _, _, x, _ in part for c in x]
            ok = ok and len(set(cs)) == len(cs)
        if ok:
            same = (n_a != 2 or rank_lists[0] == rank_lists[1]) and (len(rest) != 2 or rank_lists[n_a] == rank_lists[n_a + 1])
            if explicit and same:
                return 5 if n_a == 1 and len(rest) == 1 else 6
    return 4


def _mix(*v):
    x = 0x9e3779b9
    for k in v:
        x = ((x ^ (k & 0xffffffff)) * 0x85ebca6b + 0xc2b2ae35) & 0xffffffff
        x ^= x >> 15
    return x


def make_read(r, ref, start, cigar, layout, reverse, seed, flag=0, force=None, force_fwd=None, keep=None, without=()):
    """One record (start, flag, cigar, seq, MM, ML) and its listed events [(reference position, 1: a '+' tag | 2: a '-' tag)].
    force: {reference position: base} written into SEQ where the read has a base there; force_fwd: {forward-read position: base};
    keep: f(tag index, tag, candidates) -> the candidates to list, of candidates = [(rank among the tag's bases, forward position,
    reference position or None, the base equals the reference's)]; default: every base of a '?' tag (an `N` tag: every fifth aligned base
    that matches the reference), two of every three of a '.' tag.  without: [(base, lo, hi)]: no as-sequenced `base` at the forward
    positions [lo, hi) (applied before force and force_fwd)."""
    start, flag, cigar, seq, _, _ = cases.make_read(r, ref, start, cigar, "m", reverse, seed, flag)
    L = len(seq)
    where, p, q = {}, start, 0          # index into SEQ -> reference position
    for n, op in cigar:
        if op in "M=X":
            for k in range(n):
                where[q + k] = p + k
        if op in "MDN=X":
            p += n
        if op in "MIS=X":
            q += n
    seq = list(seq)
    for base, lo, hi in without:
        for i in range(max(lo, 0), min(hi, L)):
            q = L - 1 - i if reverse else i
            if (COMP.get(seq[q]) if reverse else seq[q]) == base:
                other = "A" if base == "T" else "T"
                seq[q] = COMP[other] if reverse else other
    for q, p in where.items():
        if force and p in force:
            seq[q] = force[p]
    for i, b in (force_fwd or {}).items():
        if 0 <= i < L:
            seq[L - 1 - i if reverse else i] = COMP[b] if reverse else b
    seq = "".join(seq)
    fwd = revcomp(seq) if reverse else seq
    tags = LAYOUTS[layout]
    group_codes = {}                    # (strand, base) -> the codes that can meet on one of its calls
    for fb, s, codes, _ in tags:
        for b in ("ACGT" if fb == "N" else fb):
            have = group_codes.setdefault((s, b), [])
            have += [c for c in codes if c not in have]
    mm, ml, events, rank_lists = "", [], [], []
    for t, (fb, s, codes, mode) in enumerate(tags):
        cand = []
        for k, i in enumerate(range(L) if fb == "N" else [i for i, c in enumerate(fwd) if c == fb]):
            q = L - 1 - i if reverse else i
            p = where.get(q)
            if fwd[i] in COMP:
                cand.append((k, i, p, p is not None and seq[q] == ref[p]))
        if keep is not None:
            listed = keep(t, tags[t], cand)
        elif fb == "N":
            listed = [c for c in cand if c[3]][::5]
        elif mode == ".":
            listed = [c for n, c in enumerate(cand) if n % 3 != 2]
        else:
            listed = cand
        listed = sorted(listed)
        deltas, last = [], -1
        for k, _, _, _ in listed:
            deltas.append(k - last - 1); last = k
        rank_lists.append([c[0] for c in listed])
        mm += "%s%s%s%s%s;" % (fb, s, "".join(codes), mode, "".join(",%d" % d for d in deltas))
        for _, i, p, _ in listed:
            group = group_codes[(s, fwd[i])]
            hot = _mix(i, seed, s == "-") % len(group)
            byte = cases.ML_PATTERN[(_mix(i, seed, 7, s == "-") >> 8) % 3]
            ml += [byte if group.index(c) == hot else 2 for c in codes]
            if p is not None:
                events.append((p, 1 if s == "+" else 2))
        if mode == "." and fb != "N":
            listed_at = {c[1] for c in listed}
            events += [(c[2], 1 if s == "+" else 2) for c in cand if c[1] not in listed_at and c[2] is not None]
    return (start, flag | (16 if reverse else 0), list(cigar), seq, mm, ml), sorted(events), decode_class(tags, rank_lists)


class Layer(cases.Layer):
    """cigar_edge_cases.Layer with the layouts of this module; keeps every read's listed events and decode class by name"""

    def __init__(self, seed, ref, stride=4):
        cases.Layer.__init__(self, seed, ref)
        self.events, self.classes, self.stride, self.clean = {}, {}, stride, False

    def add(self, cigar, layout="m", reverse=None, start=None, flag=0, name=None, **kw):
        k = len(self.records)
        if start is None:
            start = self.at
            self.at += ref_span(cigar) // self.stride + 7
        rev = (k % 2 == 1) if reverse is None else reverse
        if self.clean:                      # a stretch whose reads all carry the reference's own bases
            kw["force"] = true_bases(self.ref, start, ref_span(cigar))
        rec, events, cls = make_read(self.r, self.ref, start, cigar, layout, rev, 1000 + k, flag, **kw)
        name = name or "e%05d" % k
        self.records.append(rec)
        self.names.append(name)
        self.layouts.append(layout)
        self.events[name], self.classes[name] = events, cls
        return start

    def background(self, lo, hi, depth=4, mean=400, layouts=PLAIN):
        cases.Layer.background(self, lo, hi, depth, mean, layouts)

    def clean_stretch(self, layouts, cigar, depth=3):
        """Reads of `layouts` on both strands and plain ones, all with the reference's own bases, behind everything so far.  The rows of an
        `N` tag's code exist for every primary base that holds a call on the column (the tag is observed for all four); with mismatching
        reads on the column two rows would share position, strand and code, and their order is the reference's map order."""
        lo = self.at = max(rec[0] + ref_span(rec[2]) for rec in self.records) + 10
        self.clean = True
        for layout in layouts:
            for rev in (False, True):
                self.add(cigar, layout, rev, name="clean_%s_%d" % (layout, rev))
        self.background(lo, self.at + ref_span(cigar) + 100, depth=depth)
        self.clean = False
        return lo

    def finish(self, name, contig, prefix, **kw):
        self.flagged_copies()
        c = Case(name, contig, "".join(self.ref), self, prefix, **kw)
        c.events = [self.events.get(nm, []) for nm in c.read_names]
        c.classes = [self.classes.get(nm) if lay is not None else None for nm, lay in zip(c.read_names, c.layouts)]
        assert len(c.ref) <= CONTIG_LEN and max(len(rec[3]) for rec in c.records) <= MAX_READ
        assert {0, 1} <= set(c.classes) and 4 in c.classes, "plain (class 0 / 1) and general (class 4) reads share the BAM"
        for lay, want in (("dx_m", 5), ("c_a", 5), ("dx_h_m", 6), ("h_m_a", 6), ("dx_dot", 4), ("dup_c", 4), ("dup8", 4), ("acgt", 4),
                          ("n_b", 4), ("n_b_m", 4), ("c4tags", 4), ("c4", 0), ("neg_only", 0)):
            got = {cl for cl, x in zip(c.classes, c.layouts) if x == lay}
            assert got <= {want}, (lay, got)          # (a '-' tag alone is one explicit group: the fused decoder takes it)
        assert 100 < len(c.records) < 1000, len(c.records)
        return c


def written_calls(rec):
    """From a record as written: [(tag text, mode, {forward position of every listed call})] per tag, and the as-sequenced bases."""
    start, flag, cigar, seq, mm, ml = rec
    fwd = revcomp(seq) if flag & 16 else seq
    out = []
    for part in mm.split(";")[:-1]:
        head, _, rest = part.partition(",")
        occ = list(range(len(fwd))) if head[0] == "N" else [i for i, b in enumerate(fwd) if b == head[0]]
        rank, at = -1, set()
        for d in (rest.split(",") if rest else []):
            rank += int(d) + 1
            at.add(occ[rank])
        out.append((head[:-1], head[-1], at))
    return out, fwd


def called_positions(rec):
    """the forward positions where the record holds a call: listed ones, and for a '.' tag every other base of the tag as well"""
    tags, fwd = written_calls(rec)
    out = set()
    for head, mode, at in tags:
        out |= at if mode == "?" else {i for i, b in enumerate(fwd) if b == head[0]}
    return out


def longest_run(positions):
    """the longest run of consecutive entries of `positions` (sorted slot indexes)"""
    best = run = 0
    last = None
    for p in positions:
        run = run + 1 if last is not None and p == last + 1 else 1
        best, last = max(best, run), p
    return best


def true_bases(ref, start, n):
    return {p: ref[p] for p in range(start, start + n)}


def cpg_slots(ref):
    """the focus positions of --cpg inside one interval: both halves of every CG"""
    s = "".join(ref)
    out, at = [], s.find("CG")
    while at >= 0:
        out += [at, at + 1]
        at = s.find("CG", at + 1)
    return sorted(set(out))


def step_counts(events, slots):
    """The number of a read's events that mkp_cover_reads takes in each 64-slot step: the slots are the focus positions inside the read's
    reference span, a step's events those up to its last slot's position that no earlier step took.  slots: the read's own, sorted."""
    out, at = [], 0
    for k in range(0, len(slots), 64):
        hi = slots[min(k + 63, len(slots) - 1)]
        n = at
        while n < len(events) and events[n][0] <= hi:
            n += 1
        out.append(n - at)
        at = n
    return out


def paired_columns(events):
    both = {}
    for p, bit in events:
        both[p] = both.get(p, 0) | bit
    return sum(1 for v in both.values() if v == 3)


def keep_plan(plan):
    """list exactly the events of plan = {reference position: 1 ('+' tag) | 2 ('-' tag) | 3 (both)}"""
    def keep(t, tag, cand):
        bit = 1 if tag[1] == "+" else 2
        return [c for c in cand if c[2] is not None and plan.get(c[2], 0) & bit]
    return keep


def plan_steps(slots, start, counts):
    """A plan with exactly counts[k] events in the read's k-th 64-slot step: the step's last slot first, then its first slot, then
    positions between the slots and slots in turn; past one event per position the positions get their second feature."""
    plan, lo = {}, start
    for k, n in enumerate(counts):
        chunk = slots[64 * k:64 * k + 64]
        if not chunk:
            break
        hi, inside = chunk[-1], set(chunk)
        between = [p for p in range(lo, hi + 1) if p not in inside]
        order, rest = [hi] + ([chunk[0]] if chunk[0] != hi else []), chunk[1:-1]
        for j in range(max(len(between), len(rest))):
            order += between[j:j + 1] + rest[j:j + 1]
        assert n <= 2 * len(order), "a step of %d positions cannot hold %d events" % (len(order), n)
        for p in order[:min(n, len(order))]:
            plan[p] = 1
        for p in order[:max(0, n - len(order))]:
            plan[p] = 3
        lo = hi + 1
    return plan


# ---------------------------------------------------------------------------------------------------------------------------------
STEP_EVENTS = (0, 1, 63, 64, 65, 128, 129)
PAIRED_TOTALS = (0, 1, 63, 64, 65, 130)
EVENT_SEAMS = dict(interval=1000, region=(1000, 5000))


def event_merge(prefix):
    """1. mkp_cover_reads and the overflow loop of the stream: reads whose events inside one 64-slot step number 0 / 1 / 63 / 64 / 65 /
    128 / 129 (under --cpg, where most events match no slot; with every position a slot a step holds at most 128), an event on the last
    slot of a step and the first of the next, reads with 0 / 1 / 63 / 64 / 65 / 130 columns of two features, reads where every event is
    one of a pair — 8 193 bases long, so they lie over the first and last slot of tiles of every size, the interval seams of -i 1000 and
    the ends of --region."""
    r = random.Random(111)
    ref = cases.make_ref(r, CONTIG_LEN)
    cpg = cpg_slots(ref)
    L = Layer(112, ref, stride=6)
    k = 0
    for n in STEP_EVENTS:                     # (a) --cpg: steps of 64 focus positions, about 800 bases
        for rev in (False, True):
            start, span = L.at, 2_500
            mine = [s for s in cpg if start <= s < start + span]
            counts = [3, 3, 3]
            counts[k % 2], counts[k % 2 + 1] = n, (64 if n == 64 else 2)     # (64 then 64: an iteration that takes 64, twice)
            L.add([(span, "M")], "dup8", rev, force=true_bases(ref, start, span), keep=keep_plan(plan_steps(mine, start, counts)),
                  name="cpg%03d_%d" % (n, rev))
            k += 1
    for n in STEP_EVENTS[:-1]:                # (b) every position a slot: steps of 64 bases
        for rev in (False, True):
            start, span = L.at, 400
            counts = [2, n, 64, 0, n, 1]
            L.add([(span, "M")], "dup8", rev, force=true_bases(ref, start, span),
                  keep=keep_plan(plan_steps(list(range(start, start + span)), start, counts)), name="all%03d_%d" % (n, rev))
    for n in PAIRED_TOTALS:                   # (c) n columns of two features among single ones
        for rev in (False, True):
            start, span = L.at, 620
            plan = {p: 1 for p in range(start, start + span, 3)}
            plan.update({p: 3 for p in list(range(start + 1, start + span, 4))[:n]})
            L.add([(span, "M")], "dup8", rev, force=true_bases(ref, start, span), keep=keep_plan(plan), name="pair%03d_%d" % (n, rev))
    for start, span, rev in ((300, MAX_READ, False), (700, MAX_READ, True)):
        plan = {p: 3 for p in range(start, start + span)}      # (d) every event one of a pair, over tile, interval and region seams
        L.add([(span, "M")], "dup8", rev, start, force=true_bases(ref, start, span), keep=keep_plan(plan), name="allpair_%d_%d" % (start, rev))
    for layout in ("acgt", "c_a", "h_m_a", "dup_c", "neg_only", "dx_m", "dx_h_m", "dx_dot"):   # (e) calls between the focus positions
        for rev in (False, True):
            L.add([(500, "M"), (3, "D"), (400, "M"), (2, "I"), (300, "M")], layout, rev)
    top = L.at + 2_600
    assert top < CONTIG_LEN - MAX_READ // 4
    L.background(0, top, depth=2)
    L.clean_stretch(("n_b", "n_b_m", "acgt", "dup8"), [(500, "M"), (3, "D"), (400, "M"), (2, "I"), (300, "M")], depth=2)
    c = L.finish("event_merge", "em", prefix, seams=dict(EVENT_SEAMS))
    # the shapes are there, from the events as listed
    by_cpg, by_all, pairs = set(), set(), set()
    for (start, flag, cigar, seq, mm, ml), ev, nm in zip(c.records, c.events, c.read_names):
        if nm[:3] in ("cpg", "all", "pai"):
            span = ref_span(cigar)
            by_cpg |= set(step_counts(ev, [s for s in cpg if start <= s < start + span]))
            by_all |= set(step_counts(ev, list(range(start, start + span))))
            pairs.add(paired_columns(ev))
    assert set(STEP_EVENTS) <= by_cpg and set(STEP_EVENTS[:-1]) <= by_all and set(PAIRED_TOTALS) <= pairs, (by_cpg, by_all, pairs)
    whole = [(rec, ev) for rec, ev, nm in zip(c.records, c.events, c.read_names) if nm.startswith("allpair")]
    assert len(whole) == 2 and all(len(ev) == 2 * len(rec[3]) for rec, ev in whole)
    assert all(any(rec[0] < s < rec[0] + len(rec[3]) - 1 and bool(rec[1] & 16) == rev for rec, _ in whole)
               for s in (EVENT_SEAMS["interval"], 2 * EVENT_SEAMS["interval"]) + EVENT_SEAMS["region"] for rev in (False, True))
    # a two-feature column on the first and on the last slot of a tile: each of the two reads holds a run of two-feature slots at least
    # two tiles long, wherever the tiles begin.  Slot tiles are 256 slots by default and 64 with --tile 256 (a quarter of it), both
    # with every position a slot and under --cpg; the dense kernel's tiles are 256 positions with --tile 256 and at most 4 096 by default
    for rec, ev in whole:
        paired = sorted(p for p in {p for p, _ in ev} if (p, 1) in set(ev) and (p, 2) in set(ev))
        assert paired == list(range(rec[0], rec[0] + len(rec[3])))
        in_cpg = [k for k, s in enumerate(cpg) if rec[0] <= s < rec[0] + len(rec[3])]
        assert longest_run(in_cpg) >= 2 * 256 and len(paired) >= 2 * 4_096
    assert {5, 6} <= set(c.classes)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
TRIMS = ((50, 50), (50, 0), (0, 50), (512, 1024), (4096, 1))          # --edge-filter 50 / 50,0 / 0,50 / 512,1024 / 4096,1
DECODER_STEPS = (511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)   # the step sizes of the general, FAST and SPARSE decoders, +- 1
EDGE_LAYOUTS = ("m", "h_m", "m_dot", "h_m_dot", "c_a", "dx_m", "dx_h_m", "acgt", "dup8", "neg_only", "hm", "dx_dot")


def edge_lengths():
    """read lengths a, a + 1, b, b + 1, a + b - 1, a + b, a + b + 1 of every trim, and the lengths that put L - b on a decoder step"""
    out = set()
    for a, b in TRIMS:
        out |= {a, a + 1, b, b + 1, a + b - 1, a + b, a + b + 1} | {v + b for v in DECODER_STEPS}
    return sorted(n for n in out if 0 < n <= MAX_READ)


def edge_positions(n):
    """the forward positions a - 1, a, a + 1, L - b - 1, L - b, L - b + 1 of every trim inside a read of n bases"""
    out = set()
    for a, b in TRIMS:
        out |= {a - 1, a, a + 1, n - b - 1, n - b, n - b + 1}
    return sorted(p for p in out if 0 <= p < n)


def edge_filter(prefix):
    """2. the edge-filter predicate of the three event decoders: read lengths on a, b and a + b of every trim, L - b on the decoders' step
    sizes, a called base on each side of both cuts, soft- and hard-clipped reads, '.'-mode tags, the layouts of every decode class."""
    r = random.Random(121)
    ref = cases.make_ref(r, CONTIG_LEN)
    L = Layer(122, ref, stride=12)
    k = 0
    for n in edge_lengths():
        for rev in (False, True):
            layout = EDGE_LAYOUTS[k % len(EDGE_LAYOUTS)]; k += 1
            on = {p: "C" for p in edge_positions(n)}         # a C on every cut position (the '-' tags of dx_*: their G is the next line's)
            if layout == "neg_only":
                on = {p: "G" for p in on}
            L.add([(n, "M")], layout, rev, force_fwd=on, name="len%04d_%d" % (n, rev))
    for n, lead, tail in ((100, 7, 9), (151, 60, 0), (151, 0, 60), (1_537, 49, 51), (1_600, 513, 1_025)):   # clips inside, on and over the cuts
        for layout in ("m", "c_a", "m_dot", "dup8", "h_m", "dx_m"):
            for rev in (False, True):
                ops = ([(5, "H")] if lead else []) + ([(lead, "S")] if lead else []) + [(n - lead - tail, "M")] + ([(tail, "S")] if tail else []) + [(3, "H")]
                L.add(ops, layout, rev, force_fwd={p: "C" for p in edge_positions(n)}, name="clip%04d_%d_%s_%d" % (n, lead, layout, rev))
    assert L.at + MAX_READ < CONTIG_LEN
    L.background(0, L.at + 1_000, depth=2)
    c = L.finish("edge_filter", "ef", prefix)
    lengths = {(len(rec[3]), bool(rec[1] & 16)) for rec in c.records}
    assert all((n, rev) in lengths for n in edge_lengths() for rev in (False, True))
    assert {0, 1, 2, 3, 4, 5, 6} <= set(c.classes)
    # from the records as written: every directed read holds a call on a - 1, a, a + 1, L - b - 1, L - b, L - b + 1 of every trim
    dotted, clipped = set(), set()
    for rec, nm, lay in zip(c.records, c.read_names, c.layouts):
        if nm.startswith(("len", "clip")):
            rev, n = bool(rec[1] & 16), len(rec[3])
            missing = set(edge_positions(n)) - called_positions(rec)
            assert not missing, (nm, sorted(missing))
            if any(mode == "." for _, _, _, mode in LAYOUTS[lay]):
                dotted.add(rev)
            if nm.startswith("clip"):
                clipped.add((tuple(rec[2]), lay, rev))
                assert {"S", "H"} <= {op for _, op in rec[2]}
    assert dotted == {False, True}
    assert len(clipped) == 5 * 6 * 2 and all((ops, lay, not rev) in clipped for ops, lay, rev in clipped)
    for a, b in TRIMS:            # and for every trim reads of each length on its edges exist whose cut positions lie inside them
        for n in {a, a + 1, b, b + 1, a + b - 1, a + b, a + b + 1} | {v + b for v in DECODER_STEPS}:
            assert not 0 < n <= MAX_READ or all((n, rev) in lengths for rev in (False, True))
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
CHUNK_CALLS = (63, 64, 65)
SNP_AT = 6_007          # a CpG of make_ref: the C


def keep_chunk(n, lo=512, hi=1024):
    """list exactly n bases of the read's forward chunk [lo, hi) over all tags, and every 40th base outside it"""
    def keep(t, tag, cand):
        inside = [c for c in cand if lo <= c[1] < hi]
        share = n // 4 + (1 if t < n % 4 else 0)
        assert len(inside) >= share
        return inside[:share] + [c for c in cand if not lo <= c[1] < hi][::40]
    return keep


def keep_n_at(positions):
    """the `N` tag lists the forward positions `positions` and every fifth base besides; the other tags list everything"""
    def keep(t, tag, cand):
        return cand if tag[0] != "N" else sorted(set(cand[::5]) | {c for c in cand if c[1] in positions})
    return keep


def many_tags(prefix):
    """3. reads with 8 tags, 4 codes in one tag, 4 tags on one (strand, base); 12 distinct (base, code) pairs in the run; calls of two tags
    on bases 511 / 512 of a read; 63 / 64 / 65 called positions in one 512-base chunk; `N`-base tags; a column where some reads call C
    and others A."""
    r = random.Random(131)
    ref = cases.make_ref(r, CONTIG_LEN)
    assert ref[SNP_AT] == "C" and ref[SNP_AT + 1] == "G"
    L = Layer(132, ref, stride=5)
    for layout in ("dup8", "c4", "c4tags", "chebi", "acgt", "h_m_a", "c_a", "dup_c", "dx_m", "dx_h_m", "neg_only"):
        for rev in (False, True):
            L.add([(300, "M"), (2, "D"), (400, "M"), (3, "I"), (350, "M")], layout, rev)
            L.add([(5, "S"), (620, "M"), (4, "S")], layout, not rev)
    for rev in (False, True):
        L.add([(1_100, "M")], "c_a", rev, force_fwd={511: "C", 512: "A"}, name="b511_ca_%d" % rev)
        L.add([(1_100, "M")], "c_a", rev, force_fwd={511: "A", 512: "C"}, name="b511_ac_%d" % rev)
        for n in CHUNK_CALLS:
            L.add([(1_600, "M")], "acgt", rev, keep=keep_chunk(n), name="chunk%d_%d" % (n, rev))
    for j in range(24):          # the SNP column: C (the reference's base) in half of the reads, A in the others, on both strands
        n = 60 + 5 * j
        layout = ("c_a", "acgt", "h_m_a")[j % 3]
        L.add([(n, "M")], layout, j % 4 >= 2, SNP_AT - 20 - j, force={SNP_AT: "CA"[j % 2], SNP_AT + 1: "GT"[j % 2]}, name="snp%02d" % j)
    L.background(0, L.at + 1_700, depth=2)
    L.clean_stretch(("n_b", "n_b_m", "c_a", "dup8"), [(300, "M"), (2, "D"), (400, "M"), (3, "I"), (350, "M")], depth=2)
    L.clean = True
    for rev in (False, True):       # an `N` call and a C call on bases 511 / 512
        start = L.at - 900          # (the reference's own bases: begin where it puts a C on the read's base 512)
        while ref[start + (1_100 - 1 - 512 if rev else 512)] != ("G" if rev else "C"):
            start += 1
        L.add([(1_100, "M")], "n_b_m", rev, start, keep=keep_n_at((511, 512)), name="b511_n_%d" % rev)
    L.clean = False
    c = L.finish("many_tags", "mt", prefix)
    pairs = set()
    for rec, lay in zip(c.records, c.layouts):
        if lay is not None:
            for fb, s, codes, _ in LAYOUTS[lay]:
                pairs |= {(b if s == "+" else COMP[b], code) for b in ("ACGT" if fb == "N" else fb) for code in codes}
    assert len(pairs) == 12, sorted(pairs)
    for n in CHUNK_CALLS:
        for rev in (False, True):
            rec = c.records[c.read_names.index("chunk%d_%d" % (n, rev))]
            fwd = revcomp(rec[3]) if rev else rec[3]
            called = set()
            for part in rec[4].split(";")[:-1]:
                occ, rank = [i for i, b in enumerate(fwd) if b == part[0]], -1
                for d in part.split(",")[1:]:
                    rank += int(d) + 1
                    called.add(occ[rank])
            assert sum(1 for i in called if 512 <= i < 1024) == n
    at_snp = [rec[3][SNP_AT - rec[0]] for rec, nm in zip(c.records, c.read_names) if nm.startswith("snp")]
    assert at_snp.count("C") == 12 and at_snp.count("A") == 12
    # from the records as written, on both strands: 8 tags; 4 codes in one tag; 4 tags on one (strand, base); an `N` tag
    shapes = {}
    for rec, lay in zip(c.records, c.layouts):
        if lay is not None:
            heads = [head for head, _, _ in written_calls(rec)[0]]
            rev = bool(rec[1] & 16)
            shapes.setdefault("tags8", set()).update({rev} if len(heads) == 8 else ())
            shapes.setdefault("codes4", set()).update({rev} if any(len(h) == 6 and not h[2:].isdigit() for h in heads) else ())
            shapes.setdefault("group4", set()).update({rev} if max(sum(1 for x in heads if x[:2] == h[:2]) for h in heads) == 4 else ())
            shapes.setdefault("n_tag", set()).update({rev} if any(h[0] == "N" for h in heads) else ())
    assert all(v == {False, True} for v in shapes.values()) and len(shapes) == 4, shapes
    for rev in (False, True):       # calls of two different tags on bases 511 and 512
        for nm in ("b511_ca_%d", "b511_ac_%d", "b511_n_%d"):
            tags, _ = written_calls(c.records[c.read_names.index(nm % rev)])
            on = {p: {head for head, _, at in tags if p in at} for p in (511, 512)}
            assert on[511] and on[512] and on[511] != on[512], (nm % rev, on)
    assert {5, 6} <= set(c.classes)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
WINDOW_CALLS = (63, 64, 65, 127, 128, 129)      # listed calls inside one step window: the 64-entry rank batches of the producers, +- 1
# decode class -> (layout, stored bases per step of its decoder, read length); "3d": the explicit pair with two different delta lists
SEAM_CLASSES = {0: ("m", 4096, 4200), 1: ("h_m", 4096, 4200), 2: ("m_dot", 1024, 3100), 3: ("h_m_dot", 1024, 3100), "3d": ("h_m", 1024, 3100),
                4: ("c4tags", 512, 1600)}
SEAM_WINDOW = {4096: 0, 1024: 1, 512: 1}        # which step holds the counted window
QCAP = 576                                      # MKP_QCAP, the FAST decoders' call queue


def stored(i, n, rev):
    """forward position <-> stored (SEQ) position of a read of n bases"""
    return n - 1 - i if rev else i


def fwd_span(lo, hi, n, rev):
    """the forward positions of the stored bases [lo, hi)"""
    return (n - hi, n - lo) if rev else (lo, hi)


def keep_window(count, lo, hi, n, rev, differ=False):
    """every tag lists exactly `count` bases among the stored bases [lo, hi) and every 40th candidate outside; differ: tag t skips the
    first t candidates of the window, so the tags' delta lists differ"""
    def keep(t, tag, cand):
        inside = sorted((c for c in cand if lo <= stored(c[1], n, rev) < hi), key=lambda c: stored(c[1], n, rev))
        skip = t if differ else 0
        assert len(inside) >= count + skip, (len(inside), count)
        return inside[skip:skip + count] + [c for c in cand if not lo <= stored(c[1], n, rev) < hi][::40]
    return keep


def keep_past_by_one(t, tag, cand):
    """every base of the tag, and one entry more: the list runs past the last occurrence by exactly one"""
    return cand + [(len(cand), cand[-1][1], None, False)]


def keep_all_but_first(t, tag, cand):
    return cand[t:]


def stored_calls(rec, listed_only=False):
    """per tag (or over all tags) the stored positions of the record's calls, from the record as written"""
    n, rev = len(rec[3]), bool(rec[1] & 16)
    if listed_only:
        return [{stored(i, n, rev) for i in at} for _, _, at in written_calls(rec)[0]]
    return {stored(i, n, rev) for i in called_positions(rec)}


def producer_seams(prefix):
    """4. the seams inside the producers of the three event decoders, every shape forward and reverse, one layout per decode class 0 - 4
    (SEAM_CLASSES; classes 0 / 1 reach the event decoders with MKP_FUSED=0 and under the edge filter):
    (a) exactly 63 / 64 / 65 / 127 / 128 / 129 listed calls inside one step window of the class's decoder (512, 1024 or 4096 stored
        bases), sparse calls outside it: a rank batch of exactly 64, the first batch against the reloaded ones, a list ending on a batch end;
    (b) FAST steps whose calls all lie in the step's stored bases [512, 1024), all in [0, 512), and in both (the half-step append);
    (c) the FAST queue at its capacity: an implicit-mode read whose first step leaves 63 calls queued (127 calls, all in its lower half) and
        whose next step holds 512 occurrences of the base in its first 512 stored bases: 575 entries of MKP_QCAP = 576;
    (d) SPARSE: an odd length and a length 8k + 1, the last stored base a listed call;
    (e) a delta list that runs past the last occurrence of its base by exactly one: the read leaves no calls."""
    r = random.Random(141)
    ref = cases.make_ref(r, CONTIG_LEN)
    L = Layer(142, ref, stride=16)
    for cls, (layout, step, n) in SEAM_CLASSES.items():                       # (a)
        lo = SEAM_WINDOW[step] * step
        for count in WINDOW_CALLS:
            for rev in (False, True):
                a, b = fwd_span(lo, lo + step, n, rev)
                L.add([(n, "M")], layout, rev, force_fwd={i: "C" for i in range(a, b, 3)}, keep=keep_window(count, lo, lo + step, n, rev, cls == "3d"),
                      name="win%s_%03d_%d" % (cls, count, rev))
    n = 3_100
    for layout, keep in (("m_dot", None), ("h_m_dot", None), ("h_m", keep_all_but_first)):   # (b)
        for rev in (False, True):
            gone = [("C",) + fwd_span(0, 512, n, rev), ("C",) + fwd_span(1536, 2048, n, rev)]
            L.add([(n, "M")], layout, rev, without=gone, keep=keep, name="half_%s_%d" % (layout, rev))
    n = 2_100
    for layout in ("m_dot", "h_m_dot"):                                        # (c)
        for rev in (False, True):
            on = [i for q in list(range(0, 508, 4)) + list(range(1024, 1536)) for i in (stored(q, n, rev),)]
            L.add([(n, "M")], layout, rev, without=[("C",) + fwd_span(0, 1024, n, rev)], force_fwd={i: "C" for i in on}, name="qcap_%s_%d" % (layout, rev))
    for n in (1_235, 1_601):                                                   # (d)
        for layout in ("m", "h_m"):
            for rev in (False, True):
                L.add([(n, "M")], layout, rev, force_fwd={stored(n - 1, n, rev): "C"}, name="odd%d_%s_%d" % (n, layout, rev))
    for layout in ("m", "h_m", "m_dot", "h_m_dot", "c4tags"):                  # (e)
        for rev in (False, True):
            L.add([(300, "M")], layout, rev, keep=keep_past_by_one, name="past_%s_%d" % (layout, rev))
    for rev in (False, True):                                                  # two features on one column, as every BAM of this module has
        L.add([(600, "M")], "dup_c", rev)
    assert L.at + MAX_READ < CONTIG_LEN
    L.background(0, L.at + 4_300, depth=2)
    c = L.finish("producer_seams", "ps", prefix)
    assert {0, 1, 2, 3, 4} <= set(c.classes)
    by_name = {nm: (rec, cl) for rec, nm, cl in zip(c.records, c.read_names, c.classes)}
    for cls, (layout, step, n) in SEAM_CLASSES.items():                       # from the records as written
        lo = SEAM_WINDOW[step] * step
        for count in WINDOW_CALLS:
            for rev in (False, True):
                rec, cl = by_name["win%s_%03d_%d" % (cls, count, rev)]
                per_tag = stored_calls(rec, listed_only=True)
                assert cl == (3 if cls == "3d" else cls) and len(rec[3]) == n and bool(rec[1] & 16) == rev
                assert all(sum(1 for q in at if lo <= q < lo + step) == count for at in per_tag), (cls, count, rev)
                assert all(any(not lo <= q < lo + step for q in at) for at in per_tag)
                assert cls != "3d" or per_tag[0] != per_tag[1]
    for layout in ("m_dot", "h_m_dot", "h_m"):
        for rev in (False, True):
            rec, cl = by_name["half_%s_%d" % (layout, rev)]
            halves = [sum(1 for q in stored_calls(rec) if 512 * k <= q < 512 * k + 512) for k in range(6)]
            assert cl in (2, 3) and halves[0] == 0 and halves[1] > 0 and halves[2] > 0 and halves[3] == 0 and halves[4] > 0 and halves[5] > 0, halves
    for layout in ("m_dot", "h_m_dot"):
        for rev in (False, True):
            rec, cl = by_name["qcap_%s_%d" % (layout, rev)]
            halves = [sum(1 for q in stored_calls(rec) if 512 * k <= q < 512 * k + 512) for k in range(3)]
            assert cl in (2, 3) and halves == [127, 0, 512] and halves[0] - 64 + halves[2] == QCAP - 1, halves
    for n in (1_235, 1_601):
        assert n % 2 == 1 and (n == 1_235 or n % 8 == 1)
        for layout in ("m", "h_m"):
            for rev in (False, True):
                rec, cl = by_name["odd%d_%s_%d" % (n, layout, rev)]
                assert cl in (0, 1) and len(rec[3]) == n and all(n - 1 in at for at in stored_calls(rec, listed_only=True))
    for layout in ("m", "h_m", "m_dot", "h_m_dot", "c4tags"):
        for rev in (False, True):
            rec, _ = by_name["past_%s_%d" % (layout, rev)]
            fwd = revcomp(rec[3]) if rev else rec[3]
            for part in rec[4].split(";")[:-1]:
                assert sum(int(d) + 1 for d in part.split(",")[1:]) == fwd.count(part[0]) + 1      # the last rank is the number of bases
    return c


BUILDERS = {"event_merge": event_merge, "edge_filter": edge_filter, "many_tags": many_tags, "producer_seams": producer_seams}


# ---------------------------------------------------------------------------------------------------------------------------------
# the flag sets of the device / oracle / model comparison

def flag_sets(case):
    """The command lines (without --tile, the device's own knob) every BAM runs under."""
    ref = ["--ref", case.fa]
    thr, nof = ["--filter-threshold", str(THRESHOLD)], ["--no-filtering"]
    focus = [["--include-bed", case.bed], ["--cpg"] + ref, ["--cpg", "--combine-strands"] + ref, []]
    if case.name == "edge_filter":    # every trim, plain and inverted, under every focus mode
        out = []
        for a, b in TRIMS:
            for inv in ([], ["--invert-edge-filter"]):
                text = str(a) if a == b else "%d,%d" % (a, b)
                for f in focus:
                    out.append(f + ["--edge-filter", text] + inv + (thr if len(out) % 3 == 1 else nof))
        return out
    if case.name == "producer_seams":  # no focus, unfiltered; --cpg; --filter-threshold; one edge filter (every class through its event decoder)
        return [focus[3] + nof, focus[1] + nof, focus[3] + thr, focus[3] + ["--edge-filter", "50"] + nof]
    out = [focus[0] + thr, focus[1] + nof, focus[2] + nof, focus[3] + thr,
           focus[0] + ["--combine-mods"] + nof, focus[1] + ["--combine-mods"] + thr, focus[2] + ["--combine-mods"] + thr,
           focus[3] + ["--combine-mods"] + nof]
    if case.seams:
        a, b = case.seams["region"]
        out += [focus[0] + thr + ["-i", str(case.seams["interval"])], focus[1] + nof + ["-i", str(case.seams["interval"])],
                focus[1] + thr + ["--region", "%s:%d-%d" % (case.contig, a, b)], focus[3] + thr + ["--region", "%s:%d-%d" % (case.contig, a, b)]]
    return out


def model_kwargs(case, flags):
    """-> (arguments of column_model.pileup without the edge filter, (start trim, end trim, inverted) or None)"""
    kw, k, edge, inverted = dict(threshold=None), 0, None, False
    while k < len(flags):
        f = flags[k]
        if f == "--filter-threshold":
            kw["threshold"] = float(flags[k + 1]); k += 1
        elif f == "-i":
            kw["interval"] = int(flags[k + 1]); k += 1
        elif f == "--cpg":
            kw["motif"] = ("CG", 0)
        elif f == "--combine-strands":
            kw["combine_strands"] = True
        elif f == "--combine-mods":
            kw["combine_mods"] = True
        elif f == "--include-bed":
            kw["bed"] = [(0, len(case.ref), ".")]; k += 1
        elif f == "--region":
            a, b = flags[k + 1].split(":")[1].split("-")
            kw["region"] = (int(a), int(b)); k += 1
        elif f == "--edge-filter":
            a, _, b = flags[k + 1].partition(",")
            edge = (int(a), int(b) if b else int(a)); k += 1
        elif f == "--invert-edge-filter":
            inverted = True
        elif f in ("--ref", "--shard-bp", "--tile"):
            k += 1
        else:
            assert f == "--no-filtering", f
        k += 1
    return kw, (edge + (inverted,) if edge else None)


def model_rows(cm, case, flags, walked, parsed):
    """(the rows tests/column_model.py (`cm`) gives under `flags`, the run's numbers for FLOORS).  walked / parsed: dicts that keep the
    walks and the parsed tags of this case from one flag set to the next."""
    kw, edge = model_kwargs(case, flags)
    ef = cm.EdgeFilter(*edge) if edge else None
    key = (kw["threshold"], ef)
    if key not in walked:
        walked[key] = (cm.walk(case.records, kw["threshold"], ef, parsed), cm.call_stats(case.records, ef, parsed))
    cols, (_, removed, two) = walked[key]
    rows = cm.pileup(case.records, case.ref, walked=cols, **kw)
    return rows, (len(rows), sum(1 for v in rows.values() if v[6]), two, removed)


# (rows, rows with N_diff > 0, aligned bases with two features of one read, calls removed by the edge filter) per flag set, as
# tests/column_model.py gives them on the CPU; tests/test_column_model.py holds them equal to the model's, the GPU test asks every run for
# nine tenths of them
FLOORS = {
    "event_merge": [(29858, 1703, 20356, 0), (4863, 276, 20356, 0), (2820, 261, 20356, 0), (29858, 1703, 20356, 0), (26206, 1531, 20356, 0), (2808, 140, 20356, 0), (1526, 132, 20356, 0), (26206, 1531, 20356, 0), (29858, 1703, 20356, 0), (4859, 276, 20356, 0), (1125, 54, 20356, 0), (8584, 393, 20356, 0)],
    "edge_filter": [(39641, 10741, 13909, 9937), (5734, 877, 13909, 9937), (3082, 918, 13909, 9937), (39641, 10741, 13909, 9937), (6897, 1737, 910, 96212), (2379, 352, 910, 96212), (1719, 340, 910, 96212), (6897, 1737, 910, 96212), (40800, 11478, 14338, 5112), (5904, 994, 14338, 5112), (3044, 842, 14338, 5112), (40800, 11478, 14338, 5112), (5583, 1350, 481, 101037), (1018, 133, 481, 101037), (1094, 199, 481, 101037), (5583, 1350, 481, 101037), (34477, 8227, 14341, 5087), (5911, 986, 14341, 5087), (3127, 926, 14341, 5087), (34477, 8227, 14341, 5087), (5601, 1490, 478, 101062), (1449, 213, 478, 101062), (858, 136, 478, 101062), (5601, 1490, 478, 101062), (21530, 4917, 5214, 74195), (3940, 595, 5214, 74195), (2250, 629, 5214, 74195), (21530, 4917, 5214, 74195), (23549, 5348, 7498, 51032), (5216, 827, 7498, 51032), (2790, 779, 7498, 51032), (23549, 5348, 7498, 51032), (3371, 690, 49, 103864), (1077, 144, 49, 103864), (675, 104, 49, 103864), (3371, 690, 49, 103864), (17872, 4663, 4077, 74316), (3261, 502, 4077, 74316), (1986, 508, 4077, 74316), (17872, 4663, 4077, 74316)],
    "many_tags": [(23586, 2533, 6321, 0), (5302, 415, 6321, 0), (3055, 399, 6321, 0), (23586, 2533, 6321, 0), (16755, 2069, 6321, 0), (2309, 170, 6321, 0), (1304, 164, 6321, 0), (16755, 2069, 6321, 0)],
    "producer_seams": [(43492, 29584, 314, 0), (7538, 2678, 314, 0), (38390, 25867, 314, 0), (41705, 28740, 261, 4787)],
}
