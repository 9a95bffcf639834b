"""A plain per-base model of a pileup column, for the CIGAR-edge tests (tests/cigar_edge_cases.py), the multi-tag, duplex-tag and
edge-filter tests (tests/multi_feature_cases.py) and the tests of records that share a read name (tests/shared_name_cases.py).

Pure Python + numpy; it imports neither the oracle nor modkit_amd.  It restates the reference's column loop (src/pileup/mod.rs) in one
obvious walk: for every CIGAR op of every record, for every reference base of the op, one feature.  No windows, no chunks of ops, no
prefix tables; positions are int64 / Python ints.  An op's bases are handled as one numpy slice, which is the same walk written once.

What it restates, with the reference's lines:
    records      the column loop drops secondary / supplementary / duplicate records and empty SEQ (mod.rs:783-791, util.rs:405-407);
                 htslib's pileup has already dropped unmapped, secondary, QC-fail and duplicate ones (its default mask)
    ref-skip     an alignment inside an `N` op is dropped before anything is counted, observed codes included (mod.rs:785)
    deletion     Feature::Delete on the alignment's strand (mod.rs:851-859), after the record's codes were noted (mod.rs:831-835)
    base         SEQ[qpos], complemented for a reverse record (mod.rs:612-624, 862-869); a base that is not ACGT gives no feature
                 (mod.rs:870-874)
    call         get_mod_call (read_cache.rs:214-297): the read's calls are kept per read strand and per base of SEQ (the tag's base; for an
                 `N` tag whatever base sits there, mod_bam.rs:1245-1248); the column asks with the read's base.  The four arms
                 (mod.rs:876-938): no call -> NoCall(base); a '+' call -> a feature of the read's base on the alignment's strand; a '-'
                 call -> a feature of the COMPLEMENT of the read's base on the OTHER strand's tally (mod.rs:254-259); both -> both,
                 two features of one read on one column.  A '-' tag is called with the complement's thresholds (read_cache.rs:147-150).
                 A record whose tags fail to parse gives NoCall everywhere and notes no codes
    codes        observed codes are per reference strand and primary base (add_mod_codes_for_record, read_cache.rs:299-355): a '+' tag's
                 on the alignment's strand, a '-' tag's on the other one, under the complement (read_cache.rs:181-194)
    edge filter  --edge-filter a[,b] / --invert-edge-filter: EdgeFilter::keep_position and read_can_be_trimmed (mod_bam.rs:1642-1671) over
                 forward-read positions and the SEQ length (soft clips included), applied per (strand, base) by edge_filter_positions
                 (mod_bam.rs:1075-1102).  The inferred calls of a '.' tag were made before the filter and the filtered map is Explicit,
                 so a filtered position of a '.' tag is NO call (NoCall of the base), not a canonical one.  A (strand, base) left with
                 nothing is dropped: its bases give NoCall and its codes are not observed (read_cache.rs:159-165).  A read too short
                 to trim (L <= a or L <= b), or with nothing left at all, is an error to add_record (read_cache.rs:206-210): it joins
                 the skip set, so it still counts on every column it covers — NoCall of its base, Delete under a deletion — and
                 notes no observed codes (read_cache.rs:239-240, 308-309)
    tally        Tally / add_feature (mod.rs:167-281): a forward record counts on '+', a reverse one on '-'; the focus position's
                 strand rule keeps one or both
    rows         per strand and per primary base whose tally holds at least one call: one row per observed code of that base
                 (mod.rs:283-365), ordered by strand then code (mod.rs:440-443); N_diff = the NoCalls and the calls of every other base
                 (mod.rs:198-223), N_nocall = the NoCalls of the row's base.  One (position, strand) may give rows of two primary bases.
                 Where two of them share a code (an `N` tag's) their order is the reference's map order: the model raises
    combine-mods one row per (position, strand, primary base), coded with the base: N_mod = every modified call, N_other = 0
                 (PileupNumericOptions::Combine, mod.rs:366-407); the calls themselves are unchanged
    --include-bed  the BED's spans replace the contigs (and a --region's ends) as the stretches to work on (position_filter.rs:103-210)
    focus        the reference works in intervals of `-i` bases (interval_chunks.rs:563-632) and looks for motif hits in the text of
                 one interval only (fasta.rs:190-228), so a motif cut by an interval or region end is not a focus position; with
                 --combine-strands the interval is first extended over the motif at its end (fasta.rs:92-188)
    combine      --combine-strands adds the '-' rows at the motif's other position to the '+' rows, per code, inside one interval
                 (mod.rs:469-561)

    read names   the read cache is keyed by read NAME and built anew for every interval (ReadCache, read_cache.rs:24-43; one per
                 process_region call, mod.rs:745).  shared_walk() restates it for the names that repeat, with nothing worked out in
                 advance: for every interval the columns the reference visits (every position without a focus, the focus positions of
                 either strand with one: PileupIter, mod.rs:761-763), ascending; at each column the kept records in file order, those
                 with a base or a deletion there (a record inside an `N` op is never asked, mod.rs:785).  The first record asked about
                 a name is parsed, filtered by the edge filter with ITS OWN length and called (add_record, read_cache.rs:111-211): it
                 answers for the name until the interval ends.  A later record's feature is calls[mod strand][the ASKING record's read
                 base].get(column) of that entry (get_mod_call, read_cache.rs:214-297) through the same four arms, on the asking
                 record's alignment strand; its observed codes are the entry's, filed by the OWNER's reference strand
                 (read_cache.rs:181-194, 299-355).  An owner that fails to parse, or is left with nothing by the edge filter, puts the
                 NAME into the skip set (read_cache.rs:272-277): every record of the name is NoCall of its own base or Delete, no codes
    partition    pileup(..., keys=[...]): one key per record.  Feature vectors and observed codes are per key (mod.rs:795-835); the
                 read cache is ONE for all keys (mod.rs:745), asked by name alone.  Rows come back per key

Scope: tags of any number of primary bases on either read strand (`C+m?`, `C+h?;C+m?;A+a?`, `C+m?;G-m?`, `C+m?;C-g?`, `N+b?`, ...),
'?' and '.' modes, a caller that is --no-filtering or one --filter-threshold (the call class comes from tests/caller_model.py; a call
whose class depends on the map's iteration order raises), --edge-filter / --invert-edge-filter, --combine-mods, records that share a
read name (names that repeat take shared_walk(), unique ones the vectorised walk()), partition keys as far as one key per record with
the cache shared over the keys.
Out of scope: two motifs, --ignore, sampling, how a partition key is read from a record's tags, and max-depth.
"""
import bisect
import re

import numpy as np

import caller_model

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
COUNTS = ("n_valid", "n_mod", "n_canonical", "n_other", "n_delete", "n_fail", "n_diff", "n_nocall")
DROP_FLAGS = 4 | 256 | 512 | 1024 | 2048

# feature kinds of one (position, strand)
K_SKIP, K_DELETE, K_FAIL, K_NOCALL, K_CANONICAL, K_MOD, K_OBSERVED = -1, 0, 1, 2, 6, 10, 64   # K_NOCALL / K_CANONICAL + "ACGT".index(base); K_MOD / K_OBSERVED + index of the (base, code) pair
N_KINDS = 128


QUAL_PROBS = caller_model.quals_to_probs(np.arange(256))   # the probability of every ML byte


def code_key(code):
    """Sort key of a code as ModCodeRepr orders them (mod_base_code.rs: Code(char) before ChEbi(u32))."""
    return (1, int(code), "") if code.isdigit() else (0, 0, code)


class EdgeFilter:
    """EdgeFilter (mod_bam.rs:1634-1672) over forward-read positions and the SEQ length."""

    def __init__(self, start, end, inverted=False):
        self.start, self.end, self.inverted = int(start), int(end), bool(inverted)

    def read_can_be_trimmed(self, length):          # mod_bam.rs:1668-1671
        return not (length <= self.start or length <= self.end)

    def keep_position(self, p, length):             # mod_bam.rs:1642-1665 (the caller has checked read_can_be_trimmed)
        if self.inverted:
            return p < self.start or p >= length - self.end
        return p >= self.start and p < length - self.end

    def __hash__(self):
        return hash((self.start, self.end, self.inverted))

    def __eq__(self, o):
        return isinstance(o, EdgeFilter) and (self.start, self.end, self.inverted) == (o.start, o.end, o.inverted)


def parse_tags(mm, ml, fwd):
    """MM / ML of one record over its as-sequenced bases `fwd` -> {(read strand '+' | '-', base of SEQ): {forward position: {code: f32
    probability}}} (ModBaseInfo::new, get_base_mod_probs, mod_bam.rs:1213-1295, 1488-1535), or None when the record is one the
    reference skips: no tags, a mode it does not allow, a list that runs past the read or the ML, a listed base of SEQ that is not ACGT,
    an inferred ('.' mode) call meeting a listed one of another tag, probabilities of several tags summing above 1.01, ML bytes left
    over.  A call is filed under the base SEQ holds at its position, which for an `N` tag is whatever base is there."""
    if not mm:
        return None
    groups, at = {}, 0
    for part in [p for p in mm.split(";") if p]:
        head, _, rest = part.partition(",")
        m = re.fullmatch(r"([ACGTN])([+-])([a-z]+|[0-9]+)([?.]?)", head)
        if m is None or m.group(4) == "":          # (no mode: implicit by default, refused without --force-allow-implicit)
            return None
        fb, strand = m.group(1), m.group(2)
        codes = [m.group(3)] if m.group(3).isdigit() else list(m.group(3))
        if len(set(codes)) != len(codes):
            raise ValueError("out of the model's scope: a code listed twice in one tag")
        deltas = [int(x) for x in rest.split(",")] if rest else []
        occ = range(len(fwd)) if fb == "N" else [i for i, c in enumerate(fwd) if c == fb]
        tag, rank = {}, -1                          # forward position -> (probabilities, inferred)
        for d in deltas:
            rank += d + 1
            if rank >= len(occ) or at + len(codes) > len(ml):
                return None
            if fwd[occ[rank]] not in COMP:          # DnaBase::try_from(forward_sequence[position])? (mod_bam.rs:1245)
                return None
            tag[occ[rank]] = ({c: QUAL_PROBS[ml[at + j]] for j, c in enumerate(codes)}, False)
            at += len(codes)
        if m.group(4) == "." and fb != "N":         # (an `N` tag's converter holds no counts: nothing is inferred, mod_bam.rs:668-669)
            for p in occ:
                tag.setdefault(p, ({c: np.float32(0) for c in codes}, True))
        for p, (probs, inferred) in tag.items():
            group = groups.setdefault((strand, fwd[p]), {})
            if p not in group:
                group[p] = (dict(probs), inferred)
                continue
            have, was_inferred = group[p]
            if was_inferred != inferred:            # combine_checked: ExplicitConflictInferred (mod_bam.rs:630-634)
                return None
            for c, v in probs.items():
                have[c] = np.float32(have.get(c, np.float32(0)) + v)
            if np.float32(sum(have.values(), np.float32(0))) > caller_model.MAX_PROB:
                return None
    if at != len(ml):
        return None
    return {k: {p: probs for p, (probs, _) in g.items()} for k, g in groups.items()}


def call_classes(calls, threshold, base="C"):
    """{forward position: 'F' (filtered) | '-' (canonical) | code} through caller_model.evaluate, grouped by the codes a call lists.
    base: the base the calls are made on (the tag's base, complemented for a '-' tag: read_cache.rs:147-150)."""
    groups = {}
    for p, probs in calls.items():
        groups.setdefault(tuple(probs), []).append(p)
    out = {}
    for codes, ps in groups.items():
        P = np.array([[calls[p][c] for c in codes] for p in ps], dtype=np.float32)
        ev = caller_model.evaluate(list(codes), P, base=base, default=0.0 if threshold is None else threshold)
        if ev["order_dep"].any():
            raise ValueError("a call's class depends on the map's iteration order; the model does not decide it")
        for p, c in zip(ps, ev["cls"]):
            out[p] = "F" if c == caller_model.FILTERED else "-" if c == caller_model.CANONICAL else ev["out_codes"][c]
    return out


def motif_hits(text, start, motif, offset):
    """find_motif_hits (motif_bed.rs:288-337) over one piece of reference text that begins at `start`: ([+ positions], [- positions])."""
    iupac = {"A": "A", "C": "C", "G": "G", "T": "T", "N": "[ACGT]", "R": "[AG]", "Y": "[CT]", "D": "[AGT]", "H": "[ACT]", "W": "[AT]", "S": "[CG]"}
    rc = "".join({"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "R": "Y", "Y": "R", "D": "H", "H": "D", "W": "W", "S": "S"}[c] for c in reversed(motif))
    fwd = [m.start() for m in re.finditer("(?=%s)" % "".join(iupac[c] for c in motif), text)]
    rev = fwd if rc == motif else [m.start() for m in re.finditer("(?=%s)" % "".join(iupac[c] for c in rc), text)]
    return [start + p + offset for p in fwd], [start + p + len(motif) - 1 - offset for p in rev]


def intervals(ref, region, interval, motif, combine):
    """The reference's work units over one contig: [(start, end, {position: set of strands} or None for every position)].
    motif: (text, offset) or None."""
    lo, hi = region if region else (0, len(ref))
    hi = min(hi, len(ref))
    out, start = [], lo
    while start < hi:
        end = min(start + interval, hi)
        if motif is None:
            out.append((start, end, None))
        else:
            text, offset = motif
            if combine:   # get_motif_positions_combine_strands: look past the end, extend over the motif that sits on it
                buffered = min(end + 5 * len(text), hi)
                pos, neg = motif_hits(ref[start:buffered], start, text, offset)
                spans = sorted((p, p + len(text) - offset) for p in pos + neg)
                merged = []
                for a, b in spans:
                    if merged and a <= merged[-1][1]:
                        merged[-1][1] = max(merged[-1][1], b)
                    else:
                        merged.append([a, b])
                for a, b in merged:
                    if a <= end - 1 < b:
                        end = min(b, hi)
                        break
            else:
                pos, neg = motif_hits(ref[start:end], start, text, offset)
            focus = {}
            for p in pos:
                if start <= p < end:
                    focus.setdefault(p, set()).add("+")
            for p in neg:
                if start <= p < end:
                    focus.setdefault(p, set()).add("-")
            out.append((start, end, focus))
        start = end
    return out


def bed_regions(bed, interval):
    """group_genome_intervals (position_filter.rs:103-145): the BED's spans, merged where they overlap or touch, then joined with the
    next one, gap included, until a span is longer than the interval size."""
    merged = []
    for a, b in sorted((a, b) for a, b, _ in bed):
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    out = []
    for a, b in merged:
        if out and out[-1][1] - out[-1][0] <= interval:
            out[-1][1] = b
        else:
            out.append([a, b])
    return [tuple(x) for x in out]


def filter_groups(groups, length, edge_filter):
    """edge_filter_positions per (strand, base) (mod_bam.rs:1075-1102) as add_record applies it (read_cache.rs:151-165): a group left
    with nothing is dropped; a read too short to trim loses every group, which makes it a skipped read (read_cache.rs:206-210): NoCall
    on every column, no observed codes."""
    if edge_filter is None:
        return groups
    kept = {}
    if edge_filter.read_can_be_trimmed(length):
        for k, calls in groups.items():
            calls = {p: v for p, v in calls.items() if edge_filter.keep_position(p, length)}
            if calls:
                kept[k] = calls
    return kept


def call_stats(records, edge_filter=None, cache=None):
    """(calls listed by the records the column loop keeps, calls the edge filter removed, aligned bases that carry a call of the read's '+'
    and of its '-' strand after the filter), for the floors of the tests.  cache: as for walk()."""
    listed = removed = two = 0
    for ri, (start, flag, cigar, seq, mm, ml) in enumerate(records):
        if flag & DROP_FLAGS or not seq:
            continue
        if cache is not None and ri in cache:
            groups = cache[ri]
        else:
            rev = bool(flag & 16)
            fwd = "".join(COMP.get(c, "N") for c in reversed(seq)) if rev else seq
            groups = parse_tags(mm, list(ml), fwd) or {}
            if cache is not None:
                cache[ri] = groups
        kept = filter_groups(groups, len(seq), edge_filter)
        listed += sum(len(g) for g in groups.values())
        removed += sum(len(g) for g in groups.values()) - sum(len(g) for g in kept.values())
        both = set()
        for (strand, base), calls in kept.items():
            if strand == "+" and ("-", base) in kept:
                both |= set(calls) & set(kept[("-", base)])
        if both:
            L, q = len(seq), 0
            for n, op in cigar:
                if op in "M=X":
                    two += sum(1 for p in both if q <= (L - 1 - p if flag & 16 else p) < q + n)
                if op in "MIS=X":
                    q += n
    return listed, removed, two


def walk(records, threshold, edge_filter=None, cache=None):
    """The column loop without the focus filter: {(pos, strand): int64[N_KINDS] counts per feature kind}, and the (primary base, code)
    pairs seen.  records: (start, flag, cigar, seq, mm, ml) of one contig; edge_filter: an EdgeFilter or None; cache: a dict that keeps
    the records' parsed tags from one walk of these records to the next (they depend on neither the threshold nor the filter)."""
    pairs, parsed = [], []
    for ri, (start, flag, cigar, seq, mm, ml) in enumerate(records):
        if flag & DROP_FLAGS or not seq:
            continue
        rev = bool(flag & 16)
        fwd = "".join(COMP.get(c, "N") for c in reversed(seq)) if rev else seq
        if cache is not None and ri in cache:
            groups = cache[ri]
        else:
            groups = parse_tags(mm, list(ml), fwd) or {}
            if cache is not None:
                cache[ri] = groups
        groups = filter_groups(groups, len(seq), edge_filter)
        own, opp, seen = {}, {}, ([], [])            # calls on the read's own strand / its other one; pairs seen by alignment-relative strand
        for (strand, base), calls in sorted(groups.items()):
            on = base if strand == "+" else COMP[base]       # threshold_base (read_cache.rs:147-150), the feature's primary base
            cls = call_classes(calls, threshold, on)
            for p, c in cls.items():
                (own if strand == "+" else opp)[p] = (on, c)
            for c in sorted({c for probs in calls.values() for c in probs}, key=code_key):
                if (on, c) not in pairs:
                    pairs.append((on, c))
                seen[strand == "-"].append((on, c))
        parsed.append((start, rev, cigar, seq, own, opp, seen))
    assert len(pairs) <= N_KINDS - K_OBSERVED and K_MOD + len(pairs) <= K_OBSERVED, "too many (base, code) pairs for the key layout"
    keys = []

    def kind_of(on, c):
        return K_FAIL if c == "F" else K_CANONICAL + "ACGT".index(on) if c == "-" else K_MOD + pairs.index((on, c))
    for start, rev, cigar, seq, own, opp, seen in parsed:
        L = len(seq)
        stored = np.frombuffer(seq.encode(), dtype=np.uint8)
        lut = np.full(256, K_SKIP, dtype=np.int64)
        for i, b in enumerate("ACGT"):
            lut[ord(COMP[b] if rev else b)] = K_NOCALL + i       # the read's own base: SEQ complemented for a reverse record
        feat = lut[stored]                                       # the feature of the read's own strand (mod.rs:889-937) ...
        other = np.full(L, K_SKIP, dtype=np.int64)               # ... and of its other strand, counted on the opposite tally (mod.rs:254-259)
        for p, (on, c) in own.items():
            q = L - 1 - p if rev else p
            assert feat[q] == K_NOCALL + "ACGT".index(on)
            feat[q] = kind_of(on, c)
        for p, (on, c) in opp.items():
            q = L - 1 - p if rev else p
            assert feat[q] == K_NOCALL + "ACGT".index(COMP[on]) or p in own
            if p not in own:
                feat[q] = K_SKIP                                 # (None, Some): the negative feature alone (mod.rs:919-931)
            other[q] = kind_of(on, c)                            # its base is read_base.complement()
        strand = 1 if rev else 0
        r, q = int(start), 0
        for n, op in cigar:
            if op in "M=X":
                pos = np.arange(r, r + n, dtype=np.int64)
                f = feat[q:q + n]
                keys.append(((pos * 2 + strand) * N_KINDS + f)[f != K_SKIP])
                if opp:
                    f = other[q:q + n]
                    keys.append(((pos * 2 + (1 - strand)) * N_KINDS + f)[f != K_SKIP])
            elif op == "D":
                pos = np.arange(r, r + n, dtype=np.int64)
                keys.append((pos * 2 + strand) * N_KINDS + K_DELETE)
            if op in "M=XD":          # (not N: a ref-skip alignment never reaches add_mod_codes_for_record)
                for flip in (0, 1):   # the codes of '+' tags on the alignment's strand, of '-' tags on the other (read_cache.rs:181-188)
                    for pair in seen[flip]:
                        keys.append((pos * 2 + (strand ^ flip)) * N_KINDS + K_OBSERVED + pairs.index(pair))
            if op in "M=XDN":
                r += n
            if op in "MIS=X":
                q += n
        assert q == L, "CIGAR and SEQ lengths differ"
    cols = {}
    if keys:
        k, cnt = np.unique(np.concatenate(keys), return_counts=True)
        ps, at = np.unique(k // N_KINDS, return_inverse=True)
        tallies = np.zeros((len(ps), N_KINDS), dtype=np.int64)
        tallies[at, k % N_KINDS] = cnt
        cols = {(v >> 1, "+-"[v & 1]): tallies[i] for i, v in enumerate(ps.tolist())}
    return cols, pairs


def rows_of(t, pairs, combine_mods=False):
    """add_tally_to_counts (mod.rs:283-410) for one (position, strand) tally -> {code: counts tuple in COUNTS order}.  pairs: the
    (primary base, code) pairs of the run, in the order walk() numbered them.  One row per observed code of every primary base whose
    tally holds a call; N_diff = the NoCalls and the calls of every other base (diff_calls_count, mod.rs:198-223), N_nocall = the
    NoCalls of the row's base.  combine_mods: one row per primary base, coded with the base (PileupNumericOptions::Combine,
    mod.rs:366-407)."""
    t = t.tolist()
    if not any(t[K_CANONICAL:K_OBSERVED]):                       # no call of any base: no row
        return {}
    calls = {}                                                   # primary base -> (n_canonical, {code: n})
    for bi, b in enumerate("ACGT"):
        mods = {c: t[K_MOD + i] for i, (pb, c) in enumerate(pairs) if pb == b and t[K_MOD + i]}
        if t[K_CANONICAL + bi] or mods:
            calls[b] = (t[K_CANONICAL + bi], mods)
    out = {}
    for b, (n_can, mods) in calls.items():
        bi = "ACGT".index(b)
        total = sum(mods.values())
        n_diff = sum(t[K_NOCALL + i] for i in range(4) if i != bi) + sum(c + sum(m.values()) for ob, (c, m) in calls.items() if ob != b)
        tail = (t[K_DELETE], t[K_FAIL], n_diff, t[K_NOCALL + bi])
        if combine_mods:
            rows = {b: (n_can + total, total, n_can, 0) + tail}
        else:
            rows = {c: (n_can + total, mods.get(c, 0), n_can, total - mods.get(c, 0)) + tail
                    for i, (pb, c) in enumerate(pairs) if pb == b and t[K_OBSERVED + i]}
        for c, v in rows.items():
            if c in out:
                raise ValueError("two primary bases give a row of code %r on one (position, strand): their order is not decided" % c)
            out[c] = v
    return out


def shared_entry(rec, threshold, edge_filter):
    """add_record (read_cache.rs:111-211) for the record that is asked about first: None when the name joins the skip set (tags that do
    not parse, a read too short to trim, nothing left by the edge filter), else (calls, codes) with calls = {mod strand: {base of the
    owner's read: {reference position: (primary base, class)}}} over the owner's aligned pairs (util.rs:122-145) and codes = [(reference
    strand 0 | 1, primary base, code)], the strand being the OWNER's alignment strand for a '+' tag and the other one for a '-' tag."""
    start, flag, cigar, seq, mm, ml = rec
    rev, L = bool(flag & 16), len(seq)
    fwd = "".join(COMP.get(c, "N") for c in reversed(seq)) if rev else seq
    groups = filter_groups(parse_tags(mm, list(ml), fwd) or {}, L, edge_filter)
    if not groups:
        return None
    at, r, q = {}, int(start), 0          # forward-read position -> reference position
    for n, op in cigar:
        if op in "M=X":
            for k in range(n):
                at[L - 1 - (q + k) if rev else q + k] = r + k
        if op in "M=XDN":
            r += n
        if op in "MIS=X":
            q += n
    calls, codes = {"+": {}, "-": {}}, []
    for (strand, base), group in sorted(groups.items()):
        on = base if strand == "+" else COMP[base]
        dest = calls[strand].setdefault(base, {})
        for p, c in call_classes(group, threshold, on).items():
            if p in at:
                dest[at[p]] = (on, c)
        for c in sorted({c for probs in group.values() for c in probs}, key=code_key):
            codes.append((int(rev) ^ (strand == "-"), on, c))
    return calls, codes


def shared_walk(members, start, end, visited, threshold, edge_filter, report):
    """One interval [start, end) of the column loop for the records whose names repeat.  members: [(record index, name, key, record)] in
    file order, kept records only; visited(pos): whether the reference visits the column.  -> {key: {(pos, strand 0 | 1): {kind: n}}}
    with kinds "D", "F", ("N", base), ("C", base), ("M", (base, code)), ("O", (base, code)).  Nothing is planned: the cache and the skip
    set are filled as the loop asks.  report: a dict that collects, under "asked", per record index [(interval start, owner's index,
    owner is good, frozenset of the owner's codes)], and under "touched" / "kept" / "dropped" the cells a record answered from another
    one counts in, the calls such a record found and the owner's calls at its bases that its own base did not match."""
    spans = []
    for i, name, key, (rs, flag, cigar, seq, mm, ml) in members:
        state, q = [], 0                    # per reference position of the record: index into SEQ, -1 deletion, -2 ref-skip
        for n, op in cigar:
            if op in "M=X":
                state += range(q, q + n)
            elif op in "DN":
                state += [-1 if op == "D" else -2] * n
            if op in "MIS=X":
                q += n
        assert q == len(seq), "CIGAR and SEQ lengths differ"
        spans.append((i, name, key, int(rs), bool(flag & 16), seq, state))
    record_of = {i: rec for i, _, _, rec in members}
    out, cache, skip, owner = {}, {}, set(), {}
    lo = max(start, min(s[3] for s in spans))
    hi = min(end, max(s[3] + len(s[6]) for s in spans))
    for pos in range(lo, hi):
        if not visited(pos):
            continue
        for i, name, key, rs, rev, seq, state in spans:          # file order
            if not rs <= pos < rs + len(state) or state[pos - rs] == -2:
                continue
            if name not in cache and name not in skip:            # the first record asked owns the name in this interval
                entry = shared_entry(record_of[i], threshold, edge_filter)
                owner[name] = i
                if entry is None:
                    skip.add(name)
                else:
                    cache[name] = entry
            entry = cache.get(name)
            foreign = owner[name] != i
            seen = report["asked"].setdefault(i, [])
            if not seen or seen[-1][0] != start:
                seen.append((start, owner[name], entry is not None, frozenset(entry[1]) if entry else frozenset()))
            cells = out.setdefault(key, {})

            def add(strand, kind, counts=True):
                cell = cells.setdefault((pos, strand), {})
                cell[kind] = cell.get(kind, 0) + 1
                if foreign and counts:
                    report["touched"].add((key, pos, strand))
            if entry:
                for strand, on, c in entry[1]:                    # add_mod_codes_for_record: the owner's maps as they are
                    add(strand, ("O", (on, c)), counts=False)
            aln = int(rev)
            if state[pos - rs] == -1:
                add(aln, "D")
                continue
            base = seq[state[pos - rs]]
            base = COMP.get(base) if rev else base
            found = []
            for strand in "+-" if entry else "":
                for b, at in entry[0][strand].items():
                    if pos in at:
                        if b == base:
                            found.append((strand, at[pos]))
                        elif foreign:
                            report["dropped"] += 1
            if base not in COMP:                                  # no read base: no feature (mod.rs:864-874)
                continue
            if foreign:
                report["kept"] += len(found)
            for strand, (on, c) in found:                         # a '-' call counts on the other strand's tally (mod.rs:254-259)
                add(aln ^ (strand == "-"), "F" if c == "F" else ("C", on) if c == "-" else ("M", (on, c)))
            if not found:
                add(aln, ("N", base))
    return out


def kind_index(kind, pairs):
    """the place of one of shared_walk()'s kinds in a tally of walk()'s layout"""
    if kind in ("D", "F"):
        return K_DELETE if kind == "D" else K_FAIL
    if kind[0] in "NC":
        return (K_NOCALL if kind[0] == "N" else K_CANONICAL) + "ACGT".index(kind[1])
    return (K_MOD if kind[0] == "M" else K_OBSERVED) + pairs.index(kind[1])


def new_report():
    return {"asked": {}, "touched": set(), "kept": 0, "dropped": 0}


def mixed_records(report):
    """The records that are answered from another record in some interval and whose (owner is good, owner's codes) pairs over the intervals
    they are asked in number more than one: what the device refuses (one set of codes and one status per record)."""
    return sorted(i for i, seen in report["asked"].items()
                  if any(o != i for _, o, _, _ in seen) and len({(ok, codes) for _, _, ok, codes in seen}) > 1)


def pileup(records, ref, threshold=None, motif=None, bed=None, combine_strands=False, region=None, interval=100000, walked=None,
           edge_filter=None, combine_mods=False, names=None, keys=None, report=None, walk_cache=None):
    """The bedMethyl rows of one contig: {(pos, strand, code): counts tuple in COUNTS order}; with `keys`, {key: such rows}.
    records: [(start, flag, cigar, seq, MM text, ML bytes)]; ref: the contig's text (upper case); threshold: None for --no-filtering,
    else the one --filter-threshold; motif: (text, offset) (--cpg is ("CG", 0)); bed: [(start, end, '+' | '-' | '.')] of --include-bed;
    region: (start, end) of --region; interval: -i; walked: walk(records, threshold, edge_filter) when the caller already holds it
    (without names and keys); walk_cache: with names or keys, a dict that keeps the walks of the records with unique names per key;
    edge_filter: an EdgeFilter (--edge-filter, --invert-edge-filter); combine_mods: --combine-mods; names: one read name per record
    (None: every name is unique); keys: one partition key per record; report: new_report(), filled by shared_walk()."""
    assert not (combine_strands and motif is None)
    plain = names is None and keys is None
    names = list(names) if names is not None else list(range(len(records)))
    key_of = list(keys) if keys is not None else [None] * len(records)
    kept = [i for i, rec in enumerate(records) if not (rec[1] & DROP_FLAGS) and rec[3]]
    count = {}
    for i in kept:
        count[names[i]] = count.get(names[i], 0) + 1
    members = [(i, names[i], key_of[i], records[i]) for i in kept if count[names[i]] > 1]
    shared = {i for i, _, _, _ in members}
    report = new_report() if report is None else report
    assert walked is None or plain
    by_key, cache = {}, {} if walk_cache is None else walk_cache
    for key in sorted(set(key_of) if keys is not None else {None}, key=lambda k: (k is None, k)):
        if plain:
            cols, pairs = walked or walk(records, threshold, edge_filter)
        else:
            if key not in cache:
                cache[key] = walk([rec for i, rec in enumerate(records) if key_of[i] == key and i not in shared], threshold, edge_filter)
            cols, pairs = cache[key]
        by_pos = {}
        for (pos, strand), t in cols.items():
            by_pos.setdefault(pos, {})[strand] = t
        by_key[key] = (by_pos, sorted(by_pos), list(pairs), {})
    regions = [region]
    if bed is not None:   # --include-bed replaces the records to work on, a --region's ends included, by the BED's own spans
        regions = bed_regions(bed, interval)      # (optimize_reference_records, position_filter.rs:103-210)
    for start, end, focus in (u for reg in regions for u in intervals(ref, reg, interval, motif, combine_strands)):
        def allowed(pos):
            ok = {"+", "-"} if focus is None else focus.get(pos, set())
            if bed is not None:
                ok = ok & {s for a, b, st in bed if a <= pos < b for s in ("+-" if st == "." else st)}
            return ok
        extra = shared_walk(members, start, end, allowed, threshold, edge_filter, report) if members else {}
        for key, (by_pos, ordered, pairs, rows) in by_key.items():
            cells = {}                            # the records answered through the name cache, added to the others' tallies
            for (pos, strand), kinds in extra.get(key, {}).items():
                for kind in kinds:
                    if kind[0] in "MO" and kind[1] not in pairs:
                        pairs.append(kind[1])
                assert K_MOD + len(pairs) <= K_OBSERVED, "too many (base, code) pairs for the key layout"
                t = np.zeros(N_KINDS, dtype=np.int64)
                for kind, n in kinds.items():
                    t[kind_index(kind, pairs)] += n
                cells.setdefault(pos, {})["+-"[strand]] = t
            here, inside = {}, ordered[bisect.bisect_left(ordered, start):bisect.bisect_left(ordered, end)]
            for pos in sorted(set(inside) | set(cells)) if cells else inside:
                for strand in sorted(allowed(pos)):
                    parts = [d[pos][strand] for d in (by_pos, cells) if strand in d.get(pos, ())]
                    if parts:
                        for code, counts in rows_of(parts[0] if len(parts) == 1 else parts[0] + parts[1], pairs, combine_mods).items():
                            here[(pos, strand, code)] = counts
            if not combine_strands:
                rows.update(here)
                continue
            text, offset = motif
            codes = sorted({b for b, _ in pairs} if combine_mods else {c for _, c in pairs}, key=code_key)
            for p in sorted(q for q, s in focus.items() if "+" in s):
                other = p + len(text) - 1 - 2 * offset
                for code in codes:
                    parts = [here[k] for k in ((p, "+", code), (other, "-", code)) if k in here]
                    if parts:
                        rows[(p, ".", code)] = tuple(sum(x) for x in zip(*parts))
    far = len(motif[0]) - 1 - 2 * motif[1] if motif else 0       # a combined row holds (pos, '+') and (pos + far, '-')
    report["rows_touched"] = sum(1 for key, (_, _, _, rows) in by_key.items() for (pos, strand, code) in rows
                                 if (strand != "-" and (key, pos, 0) in report["touched"])
                                 or (strand != "+" and (key, pos + (far if strand == "." else 0), 1) in report["touched"]))
    return {key: rows for key, (_, _, _, rows) in by_key.items()} if keys is not None else by_key[None][3]


def row_order(rows):
    """The keys of `rows` in the order the reference writes them: position, strand, code."""
    return sorted(rows, key=lambda k: (k[0], k[1], code_key(k[2])))


def read_bedmethyl(path):
    """A bedMethyl file -> {(pos, strand, code): counts tuple in COUNTS order} per contig: {contig: rows}.  Header lines are skipped."""
    out = {}
    with open(path) as f:
        for ln in f:
            c = ln.split()
            if not c or c[0].startswith("#") or c[0] == "chrom":
                continue
            key = (int(c[1]), c[5], c[3].split(",")[0])
            rows = out.setdefault(c[0], {})
            assert key not in rows, "two rows for %r" % (key,)
            rows[key] = (int(c[9]), int(c[11]), int(c[12]), int(c[13]), int(c[14]), int(c[15]), int(c[16]), int(c[17]))
    return out


def first_difference(got, want, got_name="got", want_name="model"):
    """None, or (key, got counts or None, want counts or None) of the first row that differs."""
    for k in row_order(set(got) | set(want)):
        if got.get(k) != want.get(k):
            return k, got.get(k), want.get(k)
    return None


def covering(records, pos):
    """The reads over reference position `pos`, for failure reports: [(record index, start, flag, op index, op, window of 256 ops)]."""
    out = []
    for i, (start, flag, cigar, seq, mm, ml) in enumerate(records):
        r = start
        for k, (n, op) in enumerate(cigar):
            if op in "M=XDN":
                if r <= pos < r + n:
                    out.append((i, start, flag, k, "%d%s" % (n, op), k // 256))
                    break
                r += n
    return out
