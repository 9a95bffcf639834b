"""A plain per-base model of a pileup column, for the CIGAR-edge tests (tests/cigar_edge_cases.py).

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
    call         the read's call at that reference position when the read base is the tag's base, else NoCall(base)
                 (read_cache.rs:214-297); a record whose tags fail to parse gives NoCall everywhere and notes no codes
    tally        Tally / add_feature (mod.rs:167-281): a forward record counts on '+', a reverse one on '-'; the focus position's
                 strand rule keeps one or both
    rows         one row per (strand, observed code) where the strand's tally holds at least one call of the primary base
                 (mod.rs:283-365), ordered by strand then code (mod.rs:440-443); N_diff = the NoCalls of other bases, N_nocall = the
                 NoCalls of the primary base
    --include-bed  the BED's spans replace the contigs (and a --region's ends) as the stretches to work on (position_filter.rs:103-210)
    focus        the reference works in intervals of `-i` bases (interval_chunks.rs:563-632) and looks for motif hits in the text of
                 one interval only (fasta.rs:190-228), so a motif cut by an interval or region end is not a focus position; with
                 --combine-strands the interval is first extended over the motif at its end (fasta.rs:92-188)
    combine      --combine-strands adds the '-' rows at the motif's other position to the '+' rows, per code, inside one interval
                 (mod.rs:469-561)

Scope: tags of one primary base on the read's own strand (`C+m?`, `C+h?;C+m?`, `C+m.`, `C+m?;C+21839?;C+h?`, ...), a caller that is
--no-filtering or one --filter-threshold (the call class comes from tests/caller_model.py), unique read names.  Sampling, edge filter,
partition tags, --combine-mods, --ignore and max-depth are not modelled.
"""
import bisect
import re

import numpy as np

import caller_model

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
COUNTS = ("n_valid", "n_mod", "n_canonical", "n_other", "n_delete", "n_fail", "n_diff", "n_nocall")
DROP_FLAGS = 4 | 256 | 512 | 1024 | 2048

# feature kinds of one (position, strand)
K_SKIP, K_DELETE, K_FAIL, K_NOCALL, K_CANONICAL, K_MOD, K_OBSERVED = -1, 0, 1, 2, 6, 7, 32   # K_NOCALL + "ACGT".index(base); K_MOD + code index
N_KINDS = 64


def code_key(code):
    """Sort key of a code as ModCodeRepr orders them (mod_base_code.rs: Code(char) before ChEbi(u32))."""
    return (1, int(code), "") if code.isdigit() else (0, 0, code)


def parse_tags(mm, ml, fwd):
    """MM / ML of one record over its as-sequenced bases `fwd` -> (base, {forward position: {code: f32 probability}}) or None when the
    record is one the reference skips (no tags, a mode it does not allow, an ML of the wrong length, a list that runs past the read,
    probabilities of several tags summing above 1.01)."""
    if not mm:
        return None
    calls, base, at = {}, None, 0
    for part in [p for p in mm.split(";") if p]:
        head, _, rest = part.partition(",")
        m = re.fullmatch(r"([ACGT])\+([a-z]+|[0-9]+)([?.]?)", head)
        if m is None or m.group(3) == "":          # (no mode: implicit by default, refused without --force-allow-implicit)
            return None
        if base is not None and m.group(1) != base:
            raise ValueError("out of the model's scope: tags of two bases")
        base = m.group(1)
        codes = [m.group(2)] if m.group(2).isdigit() else list(m.group(2))
        deltas = [int(x) for x in rest.split(",")] if rest else []
        occ = [i for i, c in enumerate(fwd) if c == base]
        tag, rank = {}, -1
        for d in deltas:
            rank += d + 1
            if rank >= len(occ) or at + len(codes) > len(ml):
                return None
            tag[occ[rank]] = {c: caller_model.quals_to_probs(ml[at + j]) for j, c in enumerate(codes)}
            at += len(codes)
        if m.group(3) == ".":
            for p in occ:
                tag.setdefault(p, {c: np.float32(0) for c in codes})
        for p, probs in tag.items():
            have = calls.setdefault(p, {})
            fresh = not have
            for c, v in probs.items():
                have[c] = np.float32(have.get(c, np.float32(0)) + v)
            if not fresh and np.float32(sum(have.values(), np.float32(0))) > caller_model.MAX_PROB:
                return None
    if at != len(ml):
        return None
    return base, calls


def call_classes(calls, threshold):
    """{forward position: 'F' (filtered) | '-' (canonical) | code} through caller_model.evaluate, grouped by the codes a call lists."""
    groups = {}
    for p, probs in calls.items():
        groups.setdefault(tuple(probs), []).append(p)
    out = {}
    for codes, ps in groups.items():
        P = np.array([[calls[p][c] for c in codes] for p in ps], dtype=np.float32)
        ev = caller_model.evaluate(list(codes), P, base="C", default=0.0 if threshold is None else threshold)
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


def walk(records, threshold):
    """The column loop without the focus filter: {(pos, strand): int64[N_KINDS] counts per feature kind}, and the codes seen.
    records: (start, flag, cigar, seq, mm, ml) of one contig."""
    all_codes, parsed = [], []
    for start, flag, cigar, seq, mm, ml in records:
        if flag & DROP_FLAGS or not seq:
            continue
        rev = bool(flag & 16)
        fwd = "".join(COMP.get(c, "N") for c in reversed(seq)) if rev else seq
        tags = parse_tags(mm, list(ml), fwd)
        cls = call_classes(tags[1], threshold) if tags else {}
        seen = sorted({c for probs in tags[1].values() for c in probs}, key=code_key) if tags else []
        for c in seen:
            if c not in all_codes:
                all_codes.append(c)
        parsed.append((start, rev, cigar, seq, tags[0] if tags else None, cls, seen))
    keys = []
    for start, rev, cigar, seq, base, cls, seen in parsed:
        L = len(seq)
        stored = np.frombuffer(seq.encode(), dtype=np.uint8)
        lut = np.full(256, K_SKIP, dtype=np.int64)
        for i, b in enumerate("ACGT"):
            lut[ord(COMP[b] if rev else b)] = K_NOCALL + i       # the read's own base: SEQ complemented for a reverse record
        feat = lut[stored]
        for p, c in cls.items():
            q = L - 1 - p if rev else p
            assert feat[q] == K_NOCALL + "ACGT".index(base)
            feat[q] = K_FAIL if c == "F" else K_CANONICAL if c == "-" else K_MOD + all_codes.index(c)
        strand = 1 if rev else 0
        r, q = int(start), 0
        for n, op in cigar:
            if op in "M=X":
                pos = np.arange(r, r + n, dtype=np.int64)
                f = feat[q:q + n]
                keys.append(((pos * 2 + strand) * N_KINDS + f)[f != K_SKIP])
            elif op == "D":
                pos = np.arange(r, r + n, dtype=np.int64)
                keys.append((pos * 2 + strand) * N_KINDS + K_DELETE)
            if op in "M=XD":          # (not N: a ref-skip alignment never reaches add_mod_codes_for_record)
                for c in seen:
                    keys.append((pos * 2 + strand) * N_KINDS + K_OBSERVED + all_codes.index(c))
            if op in "M=XDN":
                r += n
            if op in "MIS=X":
                q += n
        assert q == L, "CIGAR and SEQ lengths differ"
    cols = {}
    if keys:
        k, cnt = np.unique(np.concatenate(keys), return_counts=True)
        for key, c in zip(k.tolist(), cnt.tolist()):
            ps, kind = divmod(key, N_KINDS)
            cols.setdefault((ps >> 1, "+-"[ps & 1]), np.zeros(N_KINDS, dtype=np.int64))[kind] = c
    return cols, all_codes


def rows_of(t, codes, base="C"):
    """add_tally_to_counts for one (position, strand) tally -> {code: counts tuple in COUNTS order}"""
    n_can = int(t[K_CANONICAL])
    mods = {c: int(t[K_MOD + i]) for i, c in enumerate(codes)}
    total = sum(mods.values())
    if n_can + total == 0:
        return {}
    bi = "ACGT".index(base)
    n_diff = sum(int(t[K_NOCALL + i]) for i in range(4) if i != bi)
    out = {}
    for i, c in enumerate(codes):
        if t[K_OBSERVED + i]:
            out[c] = (n_can + total, mods[c], n_can, total - mods[c], int(t[K_DELETE]), int(t[K_FAIL]), n_diff, int(t[K_NOCALL + bi]))
    return out


def pileup(records, ref, threshold=None, motif=None, bed=None, combine_strands=False, region=None, interval=100000, walked=None):
    """The bedMethyl rows of one contig: {(pos, strand, code): counts tuple in COUNTS order}.
    records: [(start, flag, cigar, seq, MM text, ML bytes)]; ref: the contig's text (upper case); threshold: None for --no-filtering,
    else the one --filter-threshold; motif: (text, offset) (--cpg is ("CG", 0)); bed: [(start, end, '+' | '-' | '.')] of --include-bed;
    region: (start, end) of --region; interval: -i; walked: walk(records, threshold) when the caller already holds it."""
    assert not (combine_strands and motif is None)
    cols, codes = walked or walk(records, threshold)
    by_pos = {}
    for (pos, strand), t in cols.items():
        by_pos.setdefault(pos, {})[strand] = t
    ordered = sorted(by_pos)
    rows = {}
    regions = [region]
    if bed is not None:   # --include-bed replaces the records to work on, a --region's ends included, by the BED's own spans
        regions = bed_regions(bed, interval)      # (optimize_reference_records, position_filter.rs:103-210)
    for start, end, focus in (u for reg in regions for u in intervals(ref, reg, interval, motif, combine_strands)):
        here = {}
        for pos in ordered[bisect.bisect_left(ordered, start):bisect.bisect_left(ordered, end)]:
            allowed = {"+", "-"} if focus is None else focus.get(pos, set())
            if bed is not None:
                inside = {s for a, b, st in bed if a <= pos < b for s in ("+-" if st == "." else st)}
                allowed = allowed & inside
            for strand in sorted(allowed):
                if strand in by_pos[pos]:
                    for code, counts in rows_of(by_pos[pos][strand], codes).items():
                        here[(pos, strand, code)] = counts
        if not combine_strands:
            rows.update(here)
            continue
        text, offset = motif
        for p in sorted(q for q, s in focus.items() if "+" in s):
            other = p + len(text) - 1 - 2 * offset
            for code in codes:
                parts = [here[k] for k in ((p, "+", code), (other, "-", code)) if k in here]
                if parts:
                    rows[(p, ".", code)] = tuple(sum(x) for x in zip(*parts))
    return rows


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
