"""A plain per-base model of a `pileup-hemi` column, for the duplex edge tests (tests/hemi_edge_cases.py).

Pure Python + numpy; it imports neither the oracle nor modkit_amd.  It restates the reference's duplex column loop in one obvious walk:
for every CIGAR op of every record, for every reference base of the op, one feature.  No windows, no rank tables, no merged event
lists: a read's calls on the reference's '+' strand and on its '-' strand live in two plain dicts keyed by reference position, and
the partner of a '+' call is a dict lookup at negative_strand_position(pos).

What it restates, with the reference's lines:
    intervals    the feeder runs with combine_strands = true, so the work units and their focus positions are those of the plain
                 pileup under --combine-strands (column_model.intervals); a column is a position with a '+' motif hit inside the unit
                 (positions_to_motifs.get, src/pileup/duplex.rs:284-291).  One read cache per unit (duplex.rs:266-271).
    records      htslib's pileup has dropped unmapped, secondary, QC-fail and duplicate records; the loop drops secondary /
                 supplementary / duplicate ones, empty SEQ and alignments inside a ref-skip (duplex.rs:294-302)
    deletion     DuplexFeature::Delete, whatever the record's tags say (duplex.rs:305-311)
    base         SEQ[qpos] as stored, NOT complemented for a reverse record (get_forward_read_base, src/pileup/mod.rs:612-624;
                 duplex.rs:312-317); a base that is not ACGT gives no feature.  It is also the row's primary base.
    call         get_duplex_mod_call (src/read_cache.rs:423-463): the '+' half is the record's call at the position on the tag base
                 `read base` (forward record: its own-strand tags; reverse record: its opposite-strand tags on the complement), the
                 '-' half the call at negative_strand_position(pos) = pos + (len - 1 - 2 * offset) (src/find_motifs/motif_bed.rs:
                 120-140; None when that is below 0) on the other strand's tags.  Both present -> ModCall(pattern) or Filtered
                 (DuplexModCall::from_base_mod_calls, src/mod_bam.rs:1718-1753); anything missing -> NoCall(read base).
    failed tags  a record whose tags fail (ModBaseInfo::new_from_record errs, or lists no call at all: read_cache.rs:111-117) is
                 found in no map at the first position it is asked about, fails to be added, answers NoCall for that one position
                 and sits in the skip set from then on (read_cache.rs:271-294, 430-433): one NoCall per work unit, at the first
                 column the record covers with an A/C/G/T base, and nothing else but its deletions.
    tally        DuplexFeatureVector (duplex.rs:89-119); --combine-mods turns every modified element of a pattern into the primary
                 base's letter (into_combined, mod_bam.rs:1802-1829)
    rows         decode (duplex.rs:121-205): per primary base one row per pattern; n_other_pattern = the other patterns of the base,
                 n_diff = the pattern calls of other bases, n_canonical = the `-,-` count, n_fail / n_nocall of the base, n_delete of
                 the position
    writer       src/writers.rs:185-255: position, then base, then pattern (Canonical < Code(char) < ChEbi(u32), mod_bam.rs:1675-1680);
                 valid coverage = count + n_other_pattern twice, the share as `{:.2}` of an f32

Scope: `?`-mode tags of one base pair per read (`C+m?;G-m?`, `C+h?;C+m?;G-h?;G-m?`, `C+hm?;G-hm?`, ChEBI codes, `G+m?;C-m?`),
--no-filtering or one --filter-threshold (call classes from tests/caller_model.py), --cpg / --motif with a palindromic motif,
--region, -i, --include-bed, --combine-mods, unique read names.  Sampling, edge filter, --ignore, --mask and max-depth are not modelled;
input outside the scope raises.
"""
import bisect
import copy
import re

import numpy as np

import caller_model
from column_model import bed_regions, code_key, intervals, motif_hits  # noqa: F401  (motif_hits: re-exported for the tests)

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
COUNTS = ("valid_coverage", "percent", "count", "n_canonical", "n_other_pattern", "n_delete", "n_fail", "n_diff", "n_nocall")
DROP_FLAGS = 4 | 256 | 512 | 1024 | 2048
DELETED = -1
UNDECIDED = "?"
PROBS = [p for p in caller_model.quals_to_probs(np.arange(256))]      # the f32 probability of every ML byte


class OutOfScope(ValueError):
    pass


def negative_strand_position(pos, motif):
    """MotifInfo::negative_strand_position (motif_bed.rs:120-140); motif: (text, offset)."""
    text, offset = motif
    adj = pos + (len(text) - 1 - offset) - offset
    return None if adj < 0 else adj


def parse_tags(mm, ml, fwd):
    """MM / ML of one record over its as-sequenced bases -> {(mod strand '+' | '-', tag base): {forward position: {code: f32}}}, or
    None for a record the reference puts into its skip set (no tags, a header it cannot read, no mode, an ML of the wrong length, a
    delta list that runs past the read, probabilities summing above 1.01, no call listed at all)."""
    if not mm:
        return None
    groups, at, ml = {}, 0, list(ml)
    for part in [p for p in mm.split(";") if p]:
        head, _, rest = part.partition(",")
        m = re.fullmatch(r"([ACGT])([+-])([a-z]+|[0-9]+)([?.]?)", head)
        if m is None or m.group(4) == "":
            return None
        if m.group(4) == ".":
            raise OutOfScope("implicit-mode tags")
        base, strand = m.group(1), m.group(2)
        codes = [m.group(3)] if m.group(3).isdigit() else list(m.group(3))
        occ = [i for i, c in enumerate(fwd) if c == base]
        tag, rank = {}, -1
        for d in ([int(x) for x in rest.split(",")] if rest else []):
            rank += d + 1
            if rank >= len(occ) or at + len(codes) > len(ml):
                return None
            tag[occ[rank]] = {c: PROBS[ml[at + j]] for j, c in enumerate(codes)}
            at += len(codes)
        calls = groups.setdefault((strand, base), {})
        for p, probs in tag.items():
            have = calls.get(p)
            if have is None:                # the position's first tag: its map as it is
                calls[p] = probs
                continue
            for c, v in probs.items():
                have[c] = np.float32(have.get(c, np.float32(0)) + v)
            if np.float32(sum(have.values(), np.float32(0))) > caller_model.MAX_PROB:
                return None
    if at != len(ml):
        return None
    plus = {b for s, b in groups if s == "+"}
    minus = {b for s, b in groups if s == "-"}
    if len(plus) > 1 or len(minus) > 1 or (plus and minus and COMP[next(iter(plus))] != next(iter(minus))):
        raise OutOfScope("tags of more than one base pair: %s" % sorted(groups))
    if not any(groups.values()):
        return None
    return groups


def group_sizes(mm, ml, fwd):
    """(calls listed on the read's own strand, calls listed on the opposite strand) of a record whose tags parse, else None."""
    g = parse_tags(mm, ml, fwd)
    if g is None:
        return None
    return sum(len(v) for (s, _), v in g.items() if s == "+"), sum(len(v) for (s, _), v in g.items() if s == "-")


def call_classes(calls, threshold, base):
    """{forward position: 'F' (filtered) | '-' (canonical) | code} through caller_model.evaluate, grouped by the codes a call lists.
    A call whose class depends on the map's iteration order (a tie) is UNDECIDED: the model raises if a column ever uses it."""
    by_codes = {}
    for p, probs in calls.items():
        by_codes.setdefault(tuple(probs), []).append(p)
    out = {}
    for codes, ps in by_codes.items():
        P = np.array([[calls[p][c] for c in codes] for p in ps], dtype=np.float32)
        ev = caller_model.evaluate(list(codes), P, base=base, default=0.0 if threshold is None else threshold)
        for p, c, dep in zip(ps, ev["cls"], ev["order_dep"]):
            out[p] = UNDECIDED if dep else "F" if c == caller_model.FILTERED else "-" if c == caller_model.CANONICAL else ev["out_codes"][c]
    return out


def aligned_pairs(start, cigar):
    """{reference position: index into SEQ, or DELETED}, one entry per reference base of every M / = / X / D op; a ref-skip gives none."""
    out, r, q = {}, int(start), 0
    for n, op in cigar:
        if op in "M=X":
            for k in range(n):
                out[r + k] = q + k
        elif op == "D":
            for k in range(n):
                out[r + k] = DELETED
        if op in "M=XDN":
            r += n
        if op in "MIS=X":
            q += n
    return out, r, q


class Read:
    """One record as the duplex cache holds it: where its bases and deletions lie, and its calls on the reference's two strands."""

    def __init__(self, index, rec):
        start, flag, cigar, seq, mm, ml = rec
        self.index, self.start, self.seq, self.rev = index, int(start), seq, bool(flag & 16)
        self.pairs, self.end, q = aligned_pairs(start, cigar)
        assert q == len(seq), "CIGAR and SEQ lengths differ"
        fwd = "".join(COMP.get(c, "N") for c in reversed(seq)) if self.rev else seq
        self.groups = parse_tags(mm, ml, fwd)
        self.ok = self.groups is not None
        self.ref_plus, self.ref_minus = {}, {}      # reference position -> (tag base, class): filled by called()

    def called(self, threshold):
        """a copy with the calls of the record's tags classified under `threshold` and laid on the reference's two strands"""
        rd = copy.copy(self)
        rd.ref_plus, rd.ref_minus = {}, {}
        if rd.ok:
            rd._place(threshold)
        return rd

    def _place(self, threshold):
        where = {q: r for r, q in self.pairs.items() if q != DELETED}
        L = len(self.seq)
        for (strand, base), calls in self.groups.items():
            # the base the call is made on (threshold_base, read_cache.rs:147-150)
            cls = call_classes(calls, threshold, base if strand == "+" else COMP[base])
            # a forward record's own-strand tags, and a reverse record's opposite-strand tags, speak about the reference's '+' strand
            table = self.ref_plus if (strand == "+") != self.rev else self.ref_minus
            for p, c in cls.items():
                q = L - 1 - p if self.rev else p
                if q in where:
                    assert where[q] not in table, "two tags of one strand on different bases"
                    table[where[q]] = (base, c)

    def duplex_call(self, pos, x, motif, combine_mods):
        """get_duplex_mod_call for a good record at a column it covers with base x: ('P', x, a, b) | ('F', x) | ('N', x)."""
        pos_base, neg_base = (COMP[x], x) if self.rev else (x, COMP[x])
        pc = self.ref_plus.get(pos)
        pc = pc[1] if pc is not None and pc[0] == pos_base else None
        npos = negative_strand_position(pos, motif)
        if npos is None:
            return ("N", x)
        nc = self.ref_minus.get(npos)
        nc = nc[1] if nc is not None and nc[0] == neg_base else None
        if pc is None or nc is None:
            return ("N", x)
        if UNDECIDED in (pc, nc):
            raise OutOfScope("position %d: a call's class depends on the map's iteration order; the model does not decide it" % pos)
        if pc == "F" or nc == "F":
            return ("F", x)
        if combine_mods:
            pc, nc = (x if pc != "-" else pc), (x if nc != "-" else nc)
        return ("P", x, pc, nc)


def parse(records):
    """The records the column loop keeps, their tags parsed: [Read] in file order."""
    return [Read(i, rec) for i, rec in enumerate(records) if not (rec[1] & DROP_FLAGS) and rec[3]]


def load(records, threshold, parsed=None):
    """parse(records) with every call classified under `threshold`; parsed: parse(records) when the caller already holds it."""
    return [rd.called(threshold) for rd in (parsed if parsed is not None else parse(records))]


def pattern_key(pattern):
    """DuplexPattern's derived order: Canonical < Code(char) < ChEbi(u32), element by element."""
    return tuple((0, 0, "") if e == "-" else (1,) + code_key(e) for e in pattern.split(","))


def decode(features, n_delete):
    """DuplexFeatureVector::decode for one position -> {(pattern text, primary base): counts tuple in COUNTS order}."""
    rows = {}
    for base in sorted({f[1] for f in features}):
        mine = {f: c for f, c in features.items() if f[1] == base}
        patterns = {(f[2], f[3]): c for f, c in mine.items() if f[0] == "P"}
        n_diff = sum(c for f, c in features.items() if f[1] != base and f[0] == "P")
        n_can = patterns.get(("-", "-"), 0)
        n_fail = sum(c for f, c in mine.items() if f[0] == "F")
        n_nocall = sum(c for f, c in mine.items() if f[0] == "N")
        total = sum(patterns.values())
        for (a, b), c in patterns.items():
            pct = np.float32(np.float32(c) / np.float32(total)) * np.float32(100)
            rows[("%s,%s" % (a, b), base)] = (total, "%.2f" % float(pct), c, n_can, total - c, n_delete, n_fail, n_diff, n_nocall)
    return rows


def pileup_hemi(records, ref, threshold=None, motif=("CG", 0), bed=None, region=None, interval=100000, combine_mods=False, loaded=None,
                trace=None):
    """The pileup-hemi rows of one contig: {(pos, pattern, primary base): counts tuple in COUNTS order}.
    records: [(start, flag, cigar, seq, MM text, ML bytes)] in file order; ref: the contig's text (upper case); threshold: None for
    --no-filtering, else the one --filter-threshold; motif: (text, offset) (--cpg is ("CG", 0)); bed: [(start, end, '+' | '-' | '.')]
    of --include-bed; region: (start, end); interval: -i; loaded: load(records, threshold) when the caller already holds it;
    trace: a list that receives (record index, pos, feature) of every feature, for the shape assertions of the tests."""
    text, offset = motif
    rc = "".join(COMP[c] for c in reversed(text))
    if rc != text:
        raise OutOfScope("pileup-hemi needs a palindromic motif")
    reads = loaded if loaded is not None else load(records, threshold)
    regions = [region] if bed is None else bed_regions(bed, interval)
    rows = {}
    for start, end, focus in (u for reg in regions for u in intervals(ref, reg, interval, motif, True)):
        columns = sorted(p for p, strands in focus.items() if "+" in strands
                         and (bed is None or any(a <= p < b and st in ".+" for a, b, st in bed)))
        if not columns:
            continue
        features, deletes = {p: {} for p in columns}, {p: 0 for p in columns}
        for rd in reads:
            if rd.start >= end or rd.end <= start:
                continue
            asked = False                           # a failed record: has the cache of this unit been asked about it yet
            for pos in columns[bisect.bisect_left(columns, rd.start):bisect.bisect_left(columns, rd.end)]:
                q = rd.pairs.get(pos)
                if q is None:                       # inside a ref-skip
                    continue
                if q == DELETED:
                    deletes[pos] += 1
                    continue
                x = rd.seq[q]
                if x not in COMP:
                    continue
                if rd.ok:
                    f = rd.duplex_call(pos, x, motif, combine_mods)
                elif not asked:
                    asked, f = True, ("N", x)
                else:
                    continue
                features[pos][f] = features[pos].get(f, 0) + 1
                if trace is not None:
                    trace.append((rd.index, pos, f))
        for pos in columns:
            for (pattern, base), counts in decode(features[pos], deletes[pos]).items():
                assert (pos, pattern, base) not in rows, "a column in two work units"
                rows[(pos, pattern, base)] = counts
    return rows


def row_order(rows):
    """The keys of `rows` in the order the reference writes them: position, primary base, pattern."""
    return sorted(rows, key=lambda k: (k[0], k[2], pattern_key(k[1])))


def read_hemi_bed(path):
    """A pileup-hemi bedMethyl file (tabs, or --mixed-delim) -> {contig: {(pos, pattern, primary base): counts tuple in COUNTS order}}."""
    out = {}
    with open(path) as f:
        for ln in f:
            c = ln.split()
            if not c:
                continue
            assert len(c) == 18, ln
            a, b, base = c[3].split(",")
            key = (int(c[1]), "%s,%s" % (a, b), base)
            assert int(c[2]) == key[0] + 1 and c[6] == c[1] and c[7] == c[2] and c[4] == c[9] and c[5] == ".", ln
            rows = out.setdefault(c[0], {})
            assert key not in rows, "two rows for %r" % (key,)
            rows[key] = (int(c[9]), c[10]) + tuple(int(v) for v in c[11:18])
    return out


def first_difference(got, want):
    """None, or (key, got counts or None, want counts or None) of the first row that differs."""
    for k in row_order(set(got) | set(want)):
        if got.get(k) != want.get(k):
            return k, got.get(k), want.get(k)
    return None


def covering(records, pos):
    """The reads over reference position `pos`, for failure reports: [(record index, start, flag, op index, op, window of 128 ops)]."""
    out = []
    for i, (start, flag, cigar, seq, mm, ml) in enumerate(records):
        r = start
        for k, (n, op) in enumerate(cigar):
            if op in "M=XDN":
                if r <= pos < r + n:
                    out.append((i, start, flag, k, "%d%s" % (n, op), k // 128))
                    break
                r += n
    return out
