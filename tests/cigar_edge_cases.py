"""Directed modBAMs for the CIGAR -> reference mapping of the pileup kernels: reads on the edges of the slot decoder's 256-op window and
four-op lane quads, of the 64-op chunks of the event decoders, of the 16-bit / 32-bit scan switch (an op of 128 or more in a window),
of the 64-slot steps, and spliced reads whose `N` ops run from 1 kb to 400 kb over a 2.5 Mb contig; plus reads and CpG pairs that
straddle tile, interval, region and shard seams.

Every read's SEQ is built by walking its own CIGAR over the reference (about 3 % mismatches, a few `N` bases).  The ML bytes are a fixed
pseudo-random pattern over {250, 10, 140}: with --filter-threshold 0.7 a call is modified, canonical or filtered, far from the
threshold and from ties, so a mapping that is off by one occurrence changes about two thirds of the calls behind it (of a tag's first code: every
other code of a layout carries ML 2 throughout, so within one read only the first code is ever called).  Each builder
returns a Case that holds the records as written, so tests/column_model.py sees exactly what the files hold.
"""
import random

from bamfuzz import aux_bc, aux_i, aux_z, bam_header, bam_record, bgzf_write, revcomp, write_bai
from caller_truth_cases import LAYOUTS, layout_tags

ML_PATTERN = (250, 10, 140)
THRESHOLD = 0.7
WINDOW_OP_COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 255, 256, 257, 260, 511, 512, 513, 1024, 1025]
EDGE_INDEXES = ([3, 63, 255, 511], [4, 64, 256, 512])   # the last op of a lane quad / 64-op chunk / window, and the first of the next
TILE = 256


class Case:
    def __init__(self, name, contig, ref, layer, prefix, seams=None):
        records, names = layer.records, layer.names
        self.name, self.contig, self.ref, self.seams = name, contig, ref, seams or {}
        order = sorted(range(len(records)), key=lambda i: records[i][0])
        self.records = [records[i] for i in order]          # (start, flag, cigar, seq, MM, ML), file order
        self.read_names = [names[i] for i in order]
        self.layouts = [layer.layouts[i] for i in order]     # the tag layout of every record (None: a record the column loop drops)
        self.bam, self.bam_unindexed, self.fa, self.bed = prefix + ".bam", prefix + "_noidx.bam", prefix + ".fa", prefix + ".bed"
        data, idx = bam_header([(contig, len(ref))]), []
        for (start, flag, cigar, seq, mm, ml), qname in zip(self.records, self.read_names):
            aux = aux_z("MM", mm) + aux_bc("ML", ml) + (aux_i("MN", len(seq)) if flag & (256 | 2048) else b"")
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


def ref_span(cigar):
    return sum(n for n, op in cigar if op in "MDN=X")


def make_ref(r, n, cpg_every=25):
    s = [r.choice("ACGT") for _ in range(n)]
    for p in range(7, n - 1, cpg_every):
        s[p], s[p + 1] = "C", "G"
    return s


def ml_pattern(seed, n):
    x, out = (seed * 2654435761 + 12345) & 0x7fffffff, []
    for _ in range(n):
        x = (1103515245 * x + 12345) & 0x7fffffff
        out.append(ML_PATTERN[(x >> 16) % 3])
    return out


def make_read(r, ref, start, cigar, layout, reverse, seed, flag=0):
    """One record (start, flag, cigar, seq, MM, ML): SEQ from the CIGAR's walk over `ref`, every C of the as-sequenced read listed
    ('?' tags) or two of every three ('.' tags), the first code's ML from the pattern and 2 for every other code."""
    seq, p = [], start
    for n, op in cigar:
        if op in "M=X":
            for k in range(n):
                b, y = ref[p + k], r.random()
                if op == "X" or (op == "M" and y < 0.03):
                    b = r.choice([c for c in "ACGT" if c != b])
                elif op == "M" and y < 0.035:
                    b = "N"
                seq.append(b)
        elif op in "IS":
            seq.extend(r.choice("ACGT") for _ in range(n))
        if op in "MDN=X":
            p += n
    assert p <= len(ref), "read runs past the contig"
    seq = "".join(seq)
    fwd = revcomp(seq) if reverse else seq
    n_c = fwd.count("C")
    tags = layout_tags(layout)
    implicit = tags[0][1] == "."
    ranks = [i for i in range(n_c) if not implicit or i % 3 != 2]
    deltas, last = [], -1
    for k in ranks:
        deltas.append(k - last - 1); last = k
    lst = "".join(",%d" % d for d in deltas)
    first = ml_pattern(seed, len(ranks))
    mm, ml = "", []
    for t, (codes, mode) in enumerate(tags):
        mm += "C+%s%s%s;" % ("".join(codes), mode, lst)
        for v in first:
            ml += [v if t == 0 and j == 0 else 2 for j in range(len(codes))]
    return start, flag | (16 if reverse else 0), list(cigar), seq, mm, ml


def gapped_cigar(r, n_ops, special=None, lo=1, hi=9, prefix=()):
    """A CIGAR of exactly n_ops ops: `prefix` (or a soft clip when n_ops is even, so that the read begins and ends on a match), then
    match runs separated by single gap ops (D, I, sometimes N).  special: {op index: (length, op)}, on gap slots only; the ops at
    those indexes of the finished CIGAR are asserted."""
    special = special or {}
    ops = list(prefix) if prefix else [(r.randrange(1, 6), "S")] if n_ops % 2 == 0 else []
    first = len(ops)
    assert (n_ops - 1 - first) % 2 == 0, "the read would end on a gap"
    for i in range(first, n_ops):
        if i in special:
            assert (i - first) % 2 == 1, "a special op on a match slot"
            ops.append(special[i])
        elif (i - first) % 2 == 0:
            ops.append((r.randrange(lo, hi + 1), r.choice("MMM=")))
        else:
            ops.append((r.randrange(lo, min(hi, 6) + 1), r.choice("DDIIN")))
    assert len(ops) == n_ops and all(ops[i] == v for i, v in special.items())
    return ops


class Layer:
    """Collects the reads of one BAM; spreads them over the contig."""

    def __init__(self, seed, ref):
        self.r, self.ref, self.records, self.names, self.layouts, self.at = random.Random(seed), ref, [], [], [], 50

    def add(self, cigar, layout="m", reverse=None, start=None, flag=0, name=None):
        k = len(self.records)
        if start is None:
            start = self.at
            self.at += ref_span(cigar) // 2 + 17     # successive reads overlap: columns hold several reads
        rev = (k % 2 == 1) if reverse is None else reverse
        self.records.append(make_read(self.r, self.ref, start, cigar, layout, rev, 1000 + k, flag))
        self.names.append(name or "e%05d" % k)
        self.layouts.append(layout)
        return start

    def flagged_copies(self):
        """the flag bits the column loop masks out, on copies of a few reads (names of their own)"""
        for j, bit in enumerate((256, 1024, 512, 4, 2048)):
            start, flag, cigar, seq, mm, ml = self.records[(7 * j) % len(self.records)]
            self.records.append((start, flag | bit, cigar, seq, mm, ml))
            self.names.append("flag%04d_%d" % (bit, j))
            self.layouts.append(None)         # (dropped by the column loop: counts for no decode class)

    def background(self, lo, hi, depth, mean=400, layouts=("m", "h_m")):
        r = self.r
        for _ in range(max(1, (hi - lo) * depth // mean)):
            n = r.randrange(mean // 2, mean * 3 // 2)
            start = r.randrange(lo, max(lo + 1, hi - n - 40))
            a = r.randrange(20, n - 20)
            gap = r.choice([(r.randrange(1, 8), "D"), (r.randrange(1, 8), "I"), None])
            cigar = [(n, "M")] if gap is None else [(a, "M"), gap, (n - a, "M")]
            self.add(cigar, r.choice(layouts), r.random() < 0.5, start)


LAYOUT_CYCLE = ("m", "h_m", "hm", "m_dot", "chebi", "h_m_dot")
# every directed CIGAR is written once per entry: two layouts the fused slot decoder takes (decode classes 0 and 1) and two it leaves to
# mkp_cover_reads and the event decoders (classes 2 and 4), on both strands
BOTH_DECODERS = (("m", False), ("h_m", True), ("m_dot", False), ("chebi", True))
FUSED_CLASSES, EVENT_CLASSES = (0, 1), (2, 3, 4)


def op_counts_by_decoder(case):
    """({n_cigar of the counted reads in classes 0 / 1}, {n_cigar of those in classes 2-4})"""
    fused, events = set(), set()
    for (_, _, cigar, _, _, _), layout in zip(case.records, case.layouts):
        if layout is not None:
            (fused if LAYOUTS[layout][1] in FUSED_CLASSES else events).add(len(cigar))
    return fused, events


def ops_at_by_decoder(case, index):
    """({op letter at `index`} over the reads of classes 0 / 1, the same over classes 2-4)"""
    fused, events = set(), set()
    for (_, _, cigar, _, _, _), layout in zip(case.records, case.layouts):
        if layout is not None and len(cigar) > index:
            (fused if LAYOUTS[layout][1] in FUSED_CLASSES else events).add(cigar[index][1])
    return fused, events


def window_edges(prefix):
    """1. reads of n_cigar on the window / chunk / quad edges; I, D, N, P on the last op of a lane, chunk and window and on the first of
    the next; S then I in front of the same; H S ... S H; =/X only; one M.  Every CIGAR goes to both decoders."""
    r = random.Random(11)
    ref = make_ref(r, 140_000)
    L = Layer(12, ref)
    for n in WINDOW_OP_COUNTS:
        for layout, rev in BOTH_DECODERS:
            L.add(gapped_cigar(L.r, n), layout, rev)
    for op in "IDNP":
        for idxs, n_ops in zip(EDGE_INDEXES, (515, 516)):
            ops = gapped_cigar(L.r, n_ops, {i: (40 if op == "N" else 3, op) for i in idxs})
            for layout, rev in BOTH_DECODERS:
                L.add(ops, layout, rev)
    # a soft clip, then an insertion, then insertions on the edge indexes: `S I M ...` puts the gaps on odd indexes, `H S I M ...` on even ones
    for idxs, n_ops, front in zip(EDGE_INDEXES, (515, 516), ([(4, "S"), (3, "I")], [(6, "H"), (4, "S"), (3, "I")])):
        ops = gapped_cigar(L.r, n_ops, {i: (2, "I") for i in idxs}, prefix=front)
        assert [op for _, op in ops[:len(front)]] == [op for _, op in front] and all(ops[i][1] == "I" for i in idxs)
        for layout, rev in BOTH_DECODERS:
            L.add(ops, layout, rev)
            L.add(ops + [(5, "S"), (7, "H")], layout, not rev)
    for layout, rev in BOTH_DECODERS:
        L.add([(3, "H"), (4, "S"), (30, "M"), (2, "D"), (30, "M"), (5, "S"), (2, "H")], layout, rev)
        L.add([(3, "H"), (4, "S"), (30, "M"), (2, "I"), (30, "M"), (5, "S"), (2, "H")], layout, not rev)
        L.add([(20, "="), (1, "X"), (30, "="), (2, "X"), (9, "=")], layout, rev)
        L.add([(77, "M")], layout, rev)
    L.add([(77, "M")], "hm", True)
    L.add([(77, "M")], "h_m_dot", False)
    L.flagged_copies()
    return Case("window_edges", "edges", "".join(ref), L, prefix)


def scan_switch(prefix):
    """2. windows of 256 ops all 127 long, the same with one 128, a window with one op of 65 536 or more, short-op then long-op
    windows and the reverse.  Every CIGAR goes to both decoders (one layout of class 0 / 1, one of class 2+)."""
    r = random.Random(21)
    ref = make_ref(r, 900_000)
    L = Layer(22, ref)
    k = 0

    def both(ops):
        nonlocal k
        pair = (BOTH_DECODERS[0], BOTH_DECODERS[3]) if k % 2 == 0 else (BOTH_DECODERS[1], BOTH_DECODERS[2])
        for layout, rev in pair:
            L.add(ops, layout, rev)
        k += 1
    for gap in "DI":
        base = [(127, "M") if i % 2 == 0 else (127, gap) for i in range(257)]   # ops 0..255 fill the first window; op 256 ends on a match
        for where in (None, 0, 128, 255):
            ops = list(base)
            if where is not None:
                ops[where] = (128, ops[where][1])
            both(ops)
        both(base[:255])                                                           # 255 ops of 127: one window, not full
    both([(40, "M"), (3, "D"), (66_000, "M"), (2, "I"), (40, "M")])
    both([(60, "M"), (70_000, "N"), (60, "M"), (2, "D"), (50, "M")])
    short = gapped_cigar(L.r, 257)[:256]                                           # 256 ops under 10, ending on a gap
    both(short + [(300, "M"), (200, "D"), (500, "M"), (129, "I"), (300, "M")])
    long_first = [(300, "M") if i % 2 == 0 else (150, "D") for i in range(256)]
    both(long_first + gapped_cigar(L.r, 301))
    L.flagged_copies()
    return Case("scan_switch", "scan", "".join(ref), L, prefix)


def slot_steps(prefix):
    """3. spans of exactly 63 / 64 / 65 / 128 reference positions, 64-position steps that straddle a window of 256 ops, a deletion
    over a whole step"""
    r = random.Random(31)
    ref = make_ref(r, 30_000)
    L = Layer(32, ref)
    k = 0
    for span in (63, 64, 65, 128):
        for rev in (False, True):
            L.add([(span, "M")], LAYOUT_CYCLE[k % len(LAYOUT_CYCLE)], rev); k += 1
            L.add([(span - 40, "M"), (9, "D"), (31, "M")], "m", rev)
    for lead in (1, 3, 33, 63):     # one reference base per op: a window of 256 ops ends `lead` bases off a 64-position step
        ops = [(lead, "M")] + [(1, "D") if i % 2 == 0 else (1, "M") for i in range(700)]
        L.add(ops, "m", lead % 2 == 1)
        ops = [(lead, "M")] + [(1, "I") if i % 4 == 0 else (1, "D") if i % 4 == 2 else (1, "M") for i in range(700)]
        L.add(ops, "h_m", lead % 2 == 0)
    for start_off in (0, 1, 63):
        L.add([(10 + start_off, "M"), (64, "D"), (30, "M")], "m", False)
        L.add([(10 + start_off, "M"), (200, "D"), (30, "M")], "h_m", True)
    L.background(0, 6000, 4)
    L.flagged_copies()
    return Case("slot_steps", "steps", "".join(ref), L, prefix)


SPLICED_LEN = 2_500_000
SPLICED_INTERVAL = 20_000


def spliced(prefix):
    """4. spliced reads (2-6 exons of 80-600 bases, introns of 1 kb to 400 kb, spans over the 16 kb / 128 kb / 1 Mb BAI bin levels),
    reads whose introns swallow whole tiles and whole intervals, and unspliced reads at about 10x over the exons and over islands
    inside the introns"""
    r = random.Random(41)
    ref = make_ref(r, SPLICED_LEN, cpg_every=40)
    L = Layer(42, ref)
    genes = []
    at = 30_000
    for introns in ([1_000, 3_000, 9_000], [12_000, 30_000, 1_500, 60_000], [150_000, 2_000, 100_000], [400_000, 5_000],
                    [20_000, 20_000, 20_000, 20_000, 20_000], [250_000, 390_000, 1_200]):
        exons, p = [], at
        for k in range(len(introns) + 1):
            n = r.randrange(80, 601)
            exons.append((p, n))
            p += n + (introns[k] if k < len(introns) else 0)
        genes.append(exons)
        at = p + 40_000
    assert at < SPLICED_LEN
    spliced_reads = []
    for g, exons in enumerate(genes):
        for j in range(14):
            a = r.randrange(0, len(exons) - 1)
            b = r.randrange(a + 1, len(exons))
            ops = []
            for k in range(a, b + 1):
                p, n = exons[k]
                lo = r.randrange(0, n - 60) if k == a else 0           # the first exon may begin late, the last end early
                hi = r.randrange(60, n + 1) if k == b else n
                if k == a:
                    start = p + lo
                    hi = n
                    ops.append((hi - lo, "M"))
                else:
                    ops.append((exons[k][0] - (exons[k - 1][0] + exons[k - 1][1]), "N"))
                    cut = r.randrange(10, hi - 5) if hi > 30 and r.random() < 0.3 else None
                    ops += [(hi, "M")] if cut is None else [(cut, "M"), (r.randrange(1, 5), r.choice("DI")), (hi - cut, "M")]
            if ops[-1][1] in "DI":
                ops.pop()
            spliced_reads.append((start, ops, ("m", "h_m")[j % 2], j % 3 == 0))
    for start, ops, layout, rev in spliced_reads:
        L.add(ops, layout, rev, start, name="sp%05d" % len(L.records))
    islands = []
    for exons in genes:
        for p, n in exons:
            L.background(max(0, p - 700), p + n + 700, 10, mean=500)
        for (p0, n0), (p1, _) in zip(exons, exons[1:]):
            if p1 - (p0 + n0) >= 9_000:                                 # an island of ordinary reads in the middle of the intron
                mid = (p0 + n0 + p1) // 2
                L.background(mid - 1_200, mid + 1_200, 6, mean=500)
                islands.append((mid - 1_200, mid + 1_200))
    L.flagged_copies()
    c = Case("spliced", "spl", "".join(ref), L, prefix)
    c.islands = islands
    # the inner part of every intron, 32 bases clear of its ends (a deletion inside an exon shifts the rest of its read by a few bases)
    c.introns = [(s + sum(n for n, op in ops[:i] if op in "MDN=X") + 32, s + sum(n for n, op in ops[:i + 1] if op in "MDN=X") - 32)
                 for s, ops, _, _ in spliced_reads for i, (n, op) in enumerate(ops) if op == "N"]
    return c


SEAMS = {"tile": 8 * TILE, "interval": 3_000, "region_end": 5_000, "shard": 9_000}   # -i 1000, --region seams:1000-5000, --shard-bp 3000


def seams(prefix):
    """5. a D, an N and an I straddling the first position of a tile, of an interval, of a shard and the end of a region; CpG pairs whose
    + and - positions sit either side of those seams; window-edge and spliced reads over the same seams"""
    r = random.Random(51)
    ref = make_ref(r, 120_000)
    for s in SEAMS.values():
        ref[s - 1], ref[s] = "C", "G"            # C on the last position before the seam, G on the first after it
        ref[s - 4], ref[s - 3] = "C", "G"        # and a pair that ends just before it
        ref[s + 1], ref[s + 2] = "C", "G"        # and one that begins just after it
    L = Layer(52, ref)
    k = 0
    for s in SEAMS.values():
        for gap in ((5, "D"), (5, "N"), (3, "I"), (1, "D"), (700, "N")):
            for shift in (0, 2, 3):              # the gap begins `shift` bases before the seam (an I sits on it / two before it)
                for rev in (False, True):
                    a = 60 + k % 7
                    L.add([(a, "M"), gap, (80, "M")], LAYOUT_CYCLE[k % len(LAYOUT_CYCLE)], rev, s - shift - a); k += 1
        L.add(gapped_cigar(L.r, 513), "m", False, s - 900)       # a long CIGAR whose windows lie either side of the seam
        L.add(gapped_cigar(L.r, 257), "h_m", True, s - 300)
    # the scan-switch and spliced shapes over the region end, the shard cuts and many interval ends: a full window of 127-long ops (with
    # one 128), an op of more than 65 536 and a 100 kb intron, each to both decoders
    full = [(127, "M") if i % 2 == 0 else (127, "D") for i in range(257)]
    full[128] = (128, "M")
    for (layout, rev), start in zip(BOTH_DECODERS, (4_000, 4_300, 8_000, 8_200)):
        L.add(full, layout, rev, start)
    for (layout, rev), start in zip(BOTH_DECODERS, (8_700, 8_800, 8_900, 8_950)):
        L.add([(70, "M"), (100_000, "N"), (60, "M"), (2, "D"), (70, "M")], layout, rev, start)
    L.add([(50, "M"), (2, "D"), (66_000, "M")], "h_m", False, 8_500)
    L.add([(50, "M"), (2, "I"), (66_000, "M")], "m_dot", True, 8_600)
    L.background(0, 11_500, 8)
    L.flagged_copies()
    return Case("seams", "seams", "".join(ref), L, prefix, seams=dict(SEAMS))


BUILDERS = {"window_edges": window_edges, "scan_switch": scan_switch, "slot_steps": slot_steps, "spliced": spliced, "seams": seams}


# ---------------------------------------------------------------------------------------------------------------------------------
# the flag sets of the device / oracle / model comparison

def flag_sets(case):
    """The command lines (without --tile, the device's own knob) every BAM runs under; `{fa}` / `{bed}` already filled in."""
    ref = ["--ref", case.fa]
    thr = ["--filter-threshold", str(THRESHOLD)]
    focus = [["--include-bed", case.bed] + thr, ["--motif", "C", "0"] + ref + ["--no-filtering"], ["--cpg"] + ref + thr,
             ["--cpg", "--combine-strands"] + ref + ["--no-filtering"], list(thr)]
    if case.name == "spliced":
        focus = [f + ["-i", str(SPLICED_INTERVAL)] for f in focus]
    if not case.seams:
        return focus
    out = []
    for f in focus:
        out += [f + ["-i", "1000"], f + ["--region", "%s:1000-%d" % (case.contig, case.seams["region_end"])],
                f + ["-i", "1000", "--shard-bp", "3000"]]
    return out


def oracle_flags(flags):
    """the same without the device driver's knobs"""
    out, k = [], 0
    while k < len(flags):
        if flags[k] in ("--shard-bp", "--tile"):
            k += 2
            continue
        out.append(flags[k]); k += 1
    return out


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
        elif f == "--combine-strands":
            kw["combine_strands"] = True
        elif f == "--include-bed":
            kw["bed"] = [(0, len(case.ref), ".")]; k += 1
        elif f == "--region":
            a, b = flags[k + 1].split(":")[1].split("-")
            kw["region"] = (int(a), int(b)); k += 1
        elif f in ("--ref", "--shard-bp", "--tile"):
            k += 1
        else:
            assert f == "--no-filtering", f
        k += 1
    return kw
