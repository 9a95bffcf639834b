"""GPU parity of the slot decoder's split plane: mkp_call_plane writes a call plane ({listed, before} per 32 stored bases) and a base plane
({base_lo, base_hi}); a read with calls gathers its call entries and asks the base plane for ONE DWORD only under a match slot without a
listed call, every other read gathers its base entries.  One directed modBAM per case over a reference this test writes (it holds no CG
but the ones placed here, so that under --cpg --ref every read's own-strand slots are known: the C of a CpG for a forward read, the G for a
reverse read), run through the fused decoder, the event decoders (MKP_FUSED=0) and the oracle under --cpg and --preset traditional, with
one to four codes per call (the preset adds the collapsed code's ML request to the base request; three codes make four ML requests): the
three bedMethyl files must be equal byte for byte, and a re-launch on the resident shard must give back the first pass's rows.

The geometries (`SplitPlaneBam._directed`), each on forward and reverse reads (the NoCall base is complemented on a reverse read):
  offsets   unlisted match slots at query offsets 0, 16, 32, 48, 64 / 15, 31, 47, 63 of the read (offsets 0, 15, 16, 31 of a plane word, and 32
            = offset 0 of the next word), unlisted by a mismatch (every other base in turn) or by a C the delta list skips, also behind a soft clip
  tails     l_seq 1..33, 63..65, 95..97: an unlisted match slot on the read's last base and on the first base of its last, partly filled word
            (l_seq = 1: one base, which a read with calls has listed — an unlisted slot needs a second base for the call)
  mixed     reads of 70, 100, 140 and 200 own-strand slots: steps of 64 slots with listed and unlisted slots, a step without an unlisted slot
            followed by one with some and the reverse, a step without a listed call (no ML request), unlisted slots in the second and third
            step (the dword is carried across the next step's mapping) and in the last step (its store is behind the loop)
  base-entry reads   no tags, a tag without calls, a delta list that runs past its base, a probability-sum error: in the shard of the others
  gaps      a deletion and a ref-skip over slots: no base request, the feature stays Delete / none
  seqn      reads with a base that is not A/C/G/T on unlisted slots and listed calls elsewhere
and a layer of random reads over everything.  `geometry_counts` counts, from the construction alone, the slots of every geometry; the
tests assert each count before anything runs on the GPU."""
import os
import random
import subprocess

import pytest

import modkit_amd
from bamfuzz import aux_bc, aux_z, bam_header, bam_record, bgzf_write, write_bai

pytestmark = pytest.mark.gpu

CTG = "splane"
MIN_CTG_LEN = 20_000
COMP = dict(zip("ACGTNRYMKSWBDHV=", "TGCANYRKMSWVHDB="))
IUPAC = "NRYMKSWBDHV"
TAIL_LENGTHS = list(range(1, 34)) + [63, 64, 65, 95, 96, 97]
WORD_OFFSETS = (0, 15, 16, 31)
Q_EVEN, Q_ODD = [0, 16, 32, 48, 64, 80, 96], [15, 31, 47, 63, 79, 95]
LAYOUT_CODES = {"m": ["m"], "hm": ["hm"], "h_m": ["h", "m"], "hmf": ["hmf"], "hmfc": ["hmfc"]}   # the tags' codes, one entry per MM tag


def _revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


class Read:
    def __init__(self, name, start, ops, seq, rev, tagkind, layout, listed_q, group):
        self.name, self.start, self.ops, self.seq, self.rev = name, start, ops, seq, rev
        self.tagkind, self.layout, self.listed_q, self.group = tagkind, layout, listed_q, group

    @property
    def has_calls(self):
        return self.tagkind == "calls" and bool(self.listed_q)


def own_slots(ref, start, ops, rev):
    """[(reference position, kind 'M' / 'D' / 'N', stored query index)] of the focus positions of the read's own strand in its span, in order"""
    out, p, q = [], start, 0
    for n, op in ops:
        if op in "M=X":
            for k in range(n):
                x = p + k
                own = (ref[x] == "G" and x > 0 and ref[x - 1] == "C") if rev else (ref[x] == "C" and x + 1 < len(ref) and ref[x + 1] == "G")
                if own:
                    out.append((x, "M", q + k))
            p += n; q += n
        elif op in "DN":
            for x in range(p, p + n):
                own = (ref[x] == "G" and ref[x - 1] == "C") if rev else (ref[x] == "C" and ref[x + 1] == "G")
                if own:
                    out.append((x, op, q))
            p += n
        else:   # I, S
            q += n
    return out


class SplitPlaneBam:
    def __init__(self, seed, layout, n_random=150):
        self.r = random.Random(seed)
        self.layout = layout
        self.ref = []
        self.specs = []    # (group, region offset + read start, ops, rev, tagkind, layout, unlisted(j, p, kind, q) -> None | "skip" | base, force_call)
        self._directed()
        self._fill(max(0, MIN_CTG_LEN - len(self.ref)) + 64)
        self.ref = "".join(self.ref)
        span = len(self.ref)
        for k in range(n_random):
            qlen = self.r.choice([self.r.randrange(20, 200), self.r.randrange(200, 900)])
            start = self.r.randrange(8, span - qlen - qlen // 4 - 40)
            ops, left = [], qlen
            while left:
                x = self.r.random()
                if x < 0.06 and ops and ops[-1][1] == "M" and left > 1:
                    n = min(left - 1, self.r.randrange(1, 4)); ops.append((n, "I")); left -= n
                elif x < 0.12 and ops and ops[-1][1] == "M":
                    ops.append((self.r.randrange(1, 9), self.r.choice("DDN")))
                else:
                    n = min(left, self.r.randrange(1, 150)); ops.append((n, "M")); left -= n
            if ops[-1][1] in "DN":
                ops.pop()
            rate = self.r.choice([0.0, 0.1, 0.5])
            how = lambda j, p, kind, q, rate=rate: None if self.r.random() >= rate else self.r.choice(["skip", "A", "T", "N"])
            tagkind = self.r.choice(["calls"] * 8 + ["none", "empty", "runover"])
            self.specs.append(("random", start, ops, self.r.random() < 0.5, tagkind, layout, how, False))
        self.reads = [self._build(k, s) for k, s in enumerate(self.specs)]

    # ---- the reference: filler without CG, CpGs where a region places them
    def _fill(self, n):
        for _ in range(n):
            self.ref.append(self.r.choice("ACT" if self.ref and self.ref[-1] == "C" else "ACGT"))

    def _region(self, cs, length):
        off = len(self.ref)
        self._fill(length)
        for c in cs:
            self.ref[off + c], self.ref[off + c + 1] = "C", "G"
        return off

    def _slots_at(self, qs, rev, ops, group, tagkind="calls", unlisted=None, layout=None, margin=20):
        """a read with own-strand slots at the query indexes qs (match ops only in front of them), in a region of its own"""
        q_of = {}   # query index -> offset from the read's start on the reference
        p = q = 0
        for n, op in ops:
            if op in "M=X":
                for k in range(n):
                    q_of[q + k] = p + k
                p += n; q += n
            elif op in "DN":
                p += n
            else:
                q += n
        cs = [margin + q_of[x] - (1 if rev else 0) for x in qs]
        off = self._region(cs, margin + p + margin)
        self.specs.append((group, off + margin, ops, rev, tagkind, layout or self.layout, unlisted or (lambda j, p, kind, q: None), True))

    def _directed(self):
        other = {False: "AGT", True: "ACT"}   # a mismatch on a slot: any base but the one the tag counts on the stored strand
        for rev in (False, True):
            # offsets of a plane word
            for qs in (Q_EVEN, Q_ODD):
                for mode in ("mm", "skip", "clip"):
                    ops = [(100, "M")] if mode != "clip" else [(3, "S"), (97, "M")]
                    use = [x for x in qs if mode != "clip" or x >= 3]
                    unl = set(use[:-2])
                    how = (lambda j, p, kind, q, unl=unl, rev=rev, mode=mode: None if q not in unl else
                           "skip" if mode == "skip" else other[rev][(q // 15) % 3])
                    self._slots_at(use, rev, ops, "offsets", unlisted=how)
            # the last, partly filled word
            for L in TAIL_LENGTHS:
                w0 = 32 * ((L - 1) // 32)
                qs = [L - 1] if L - 1 - w0 < 2 else [w0, L - 1]
                if w0 >= 8:
                    qs = [3] + qs   # a listed call in the first word as well
                unl = set(qs) - {3} if L > 1 else set()
                how = (lambda j, p, kind, q, unl=unl, rev=rev, L=L: None if q not in unl else "skip" if (L + q) % 2 else other[rev][(L + q) % 3])
                self._slots_at(qs, rev, [(L, "M")], "tails", unlisted=how)
            # mixed steps
            mixed = [
                (200, 4, lambda j: (64 <= j < 128 and j % 7 == 0) or j >= 195),
                (100, 5, lambda j: j < 64 and j % 5 == 1),
                (140, 3, lambda j: j < 64 or j == 139),
                (70, 4, lambda j: j == 69),
            ]
            for n, step, pred in mixed:
                n_m = 5 + step * n + 5
                ops = [(n_m // 2, "M"), (2, "I"), (n_m - n_m // 2, "M")]
                qs = [5 + step * j + (2 if 5 + step * j >= n_m // 2 else 0) for j in range(n)]
                how = lambda j, p, kind, q, pred=pred, rev=rev: None if not pred(j) else "skip" if j % 2 else other[rev][j % 3]
                self._slots_at(qs, rev, ops, "mixed", unlisted=how)
            # reads that take the base entry, beside reads with calls
            for tagkind in ("none", "empty", "runover", "sumerr"):
                self._slots_at(Q_EVEN if rev else Q_ODD, rev, [(100, "M")], "base_entry", tagkind=tagkind,
                               layout="h_m" if tagkind == "sumerr" else None)
            # a deletion and a ref-skip over slots
            for gap in "DN":
                ops = [(40, "M"), (12, gap), (40, "M")]
                qs = [4 * j for j in range(1, 10)] + [40 + 4 * j for j in range(1, 10)]
                off = len(self.ref)
                self._slots_at(qs, rev, ops, "gaps", unlisted=lambda j, p, kind, q: "skip" if j % 5 == 0 else None)
                start = off + 20
                for x in (42, 46, 50):   # CpGs under the gap (reference offsets from the read's start)
                    self.ref[start + x - (1 if rev else 0)], self.ref[start + x + (0 if rev else 1)] = "C", "G"
            # a base that is not A/C/G/T on a slot, listed calls elsewhere
            self._slots_at([6 * j + 1 for j in range(16)], rev, [(100, "M")], "seqn",
                           unlisted=lambda j, p, kind, q: IUPAC[j % len(IUPAC)] if j % 4 == 0 else None)

    # ---- one read from its spec
    def _build(self, k, spec):
        group, start, ops, rev, tagkind, layout, unlisted, force_call = spec
        r, ref = self.r, self.ref
        seq, p = [], start
        for n, op in ops:
            if op in "M=X":
                seq += list(ref[p:p + n]); p += n
            elif op in "DN":
                p += n
            else:
                seq += [r.choice("ACGT") for _ in range(n)]
        assert len(seq) == sum(n for n, op in ops if op in "MIS=X") and p <= len(ref) - 2
        counted = "G" if rev else "C"
        slots = own_slots(ref, start, ops, rev)
        slot_q = {q for _, kind, q in slots if kind == "M"}
        skipped = set()
        for j, (pos, kind, q) in enumerate(slots):
            if kind != "M":
                continue
            h = unlisted(j, pos, kind, q)
            if h == "skip":
                skipped.add(q)
            elif h is not None:
                seq[q] = h
        if force_call and tagkind in ("calls", "sumerr") and not any(seq[q] == counted and q not in skipped for q in range(len(seq))):
            free = [q for q in range(len(seq)) if q not in slot_q]
            if free:
                seq[free[0]] = counted   # a call off the focus positions: the read has calls, its slots stay as placed
        listed = set()
        if tagkind in ("calls", "sumerr"):
            rate = r.choice([1.0, 0.6])
            for q, b in enumerate(seq):
                if b == counted and q not in skipped and (q in slot_q or r.random() < rate or not listed):
                    listed.add(q)
        return Read("r%05d" % k, start, ops, "".join(seq), rev, tagkind, layout, listed, group)

    def _aux(self, rd):
        r = self.r
        if rd.tagkind == "none":
            return b""
        fwd = _revcomp(rd.seq) if rd.rev else rd.seq
        L = len(fwd)
        occ = [i for i, c in enumerate(fwd) if c == "C"]
        picked = [k for k, i in enumerate(occ) if ((L - 1 - i) if rd.rev else i) in rd.listed_q] if rd.tagkind in ("calls", "sumerr") else []
        if rd.tagkind == "runover":
            picked = [k for k in range(len(occ)) if r.random() < 0.5]
        deltas, prev = [], -1
        for k in picked:
            deltas.append(k - prev - 1); prev = k
        if rd.tagkind == "runover":
            deltas.append(len(occ) - prev + r.randrange(0, 3))
        n = len(deltas)
        lst = "".join("," + str(d) for d in deltas)
        tags = LAYOUT_CODES[rd.layout]
        n_codes = sum(len(t) for t in tags)
        calls = []
        for _ in range(n):
            vals, rem = [], 255
            for _ in range(n_codes):
                v = r.choice([r.randrange(0, rem + 1), 0, rem, rem // 2]); vals.append(v); rem -= v
            r.shuffle(vals)
            calls.append(vals)
        if rd.tagkind == "sumerr" and calls:
            calls[r.randrange(n)] = [200, 200]   # (h_m) 0.783 + 0.783 > 1.01
        mm = "".join("C+%s?%s;" % (t, lst) for t in tags)
        if len(tags) == 1:
            ml = [v for c in calls for v in c]
        else:
            ml = [c[t] for t in range(len(tags)) for c in calls]
        return aux_z("MM", mm) + aux_bc("ML", ml)

    def write(self, prefix, index):
        data = bam_header([(CTG, len(self.ref))])
        recs = sorted(self.reads, key=lambda rd: rd.start)
        idx = []
        for rd in recs:
            rec = bam_record(0, rd.start, 16 if rd.rev else 0, rd.name, rd.ops, rd.seq, self._aux(rd))
            idx.append((0, rd.start, sum(n for n, op in rd.ops if op in "MDN=X"), 16 if rd.rev else 0, len(data), len(rec)))
            data += rec
        offs = bgzf_write(prefix + ".bam", bytes(data))
        if index:
            write_bai(prefix + ".bam.bai", 1, offs, idx)
        with open(prefix + ".fa", "w") as f:
            f.write(">%s\n" % CTG)
            for i in range(0, len(self.ref), 60):
                f.write(self.ref[i:i + 60] + "\n")
        return prefix + ".bam", prefix + ".fa"


def geometry_counts(bam):
    """from the construction alone: how many slots (reads, steps) of every geometry of the docstring the BAM holds"""
    c = {}

    def add(key, n=1):
        c[key] = c.get(key, 0) + n
    for rd in bam.reads:
        slots = own_slots(bam.ref, rd.start, rd.ops, rd.rev)
        L, s = len(rd.seq), "-" if rd.rev else "+"
        if not rd.has_calls:
            if slots and rd.tagkind != "calls":
                add(("base_entry", rd.tagkind, s))
            continue
        add(("reads_with_calls", s))
        unl = [kind == "M" and q not in rd.listed_q for _, kind, q in slots]
        lst = [kind == "M" and q in rd.listed_q for _, kind, q in slots]
        for (pos, kind, q), u in zip(slots, unl):
            if kind != "M":
                add(("gap_slot", kind, s))
                continue
            if not u:
                continue
            base = rd.seq[q]
            if q % 32 in WORD_OFFSETS:
                add(("unlisted_at_offset", q % 32, s))
            if q == 32:
                add(("unlisted_at_q32", s))
            if q >> 5 == (L - 1) >> 5 and L in TAIL_LENGTHS:
                add(("unlisted_in_last_word", L, s))
            if q == L - 1:
                add(("unlisted_on_last_base", s))
            if base not in "ACGT" and any(lst):
                add(("seqn_unlisted_with_listed_elsewhere", s))
            if base in "ACGT":
                add(("nocall_base", base, s))
        if L == 1 and slots:
            add(("slot_in_last_word_of_one_base", s))
        steps = [(sum(unl[i:i + 64]), sum(lst[i:i + 64])) for i in range(0, len(slots), 64)]
        for k, (nu, nl) in enumerate(steps):
            if nu and nl:
                add(("step_mixed", s))
            if nu and not nl:
                add(("step_without_listed", s))
            if k and not steps[k - 1][0] and nu:
                add(("step_none_then_some", s))
            if k and steps[k - 1][0] and not nu:
                add(("step_some_then_none", s))
            if k >= 1 and nu:
                add(("unlisted_in_second_step_or_later", s))
            if k >= 2 and nu:
                add(("unlisted_in_third_step_or_later", s))
            if k == len(steps) - 1 and k >= 1 and nu:
                add(("unlisted_in_last_step_behind_the_loop", s))
        if len(slots) > 64:
            add(("over_64_slots", s))
        if len(slots) > 128:
            add(("over_128_slots", s))
    return c


def required_keys():
    keys = []
    for s in "+-":
        keys += [("reads_with_calls", s), ("unlisted_at_q32", s), ("unlisted_on_last_base", s), ("slot_in_last_word_of_one_base", s)]
        keys += [("unlisted_at_offset", o, s) for o in WORD_OFFSETS]
        keys += [("unlisted_in_last_word", L, s) for L in TAIL_LENGTHS if L > 1]
        keys += [("step_mixed", s), ("step_without_listed", s), ("step_none_then_some", s), ("step_some_then_none", s),
                 ("unlisted_in_second_step_or_later", s), ("unlisted_in_third_step_or_later", s), ("unlisted_in_last_step_behind_the_loop", s),
                 ("over_64_slots", s), ("over_128_slots", s)]
        keys += [("base_entry", t, s) for t in ("none", "empty", "runover", "sumerr")]
        keys += [("gap_slot", "D", s), ("gap_slot", "N", s), ("seqn_unlisted_with_listed_elsewhere", s)]
        # the NoCall base of either strand's slots: every base but the one the tag counts there (a skipped C / G is that base itself)
        keys += [("nocall_base", b, s) for b in "ACGT"]
    return keys


def assert_not_vacuous(bam):
    counts = geometry_counts(bam)
    missing = [k for k in required_keys() if counts.get(k, 0) < 1]
    assert not missing, "the BAM holds no slot of: %r" % (missing,)
    assert MIN_CTG_LEN <= len(bam.ref) <= 60_000 and 200 <= len(bam.reads) <= 600
    return counts


def _oracle(oracle_bin, bam, out, flags):
    p = subprocess.run([oracle_bin, "pileup", bam, out] + flags, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-400:]
    return open(out).read()


def _device(bam, out, flags, fused):
    old = os.environ.get("MKP_FUSED")
    try:
        if fused:
            os.environ.pop("MKP_FUSED", None)
        else:
            os.environ["MKP_FUSED"] = "0"
        modkit_amd.pileup([bam, out] + flags)
    finally:
        if old is None:
            os.environ.pop("MKP_FUSED", None)
        else:
            os.environ["MKP_FUSED"] = old
    return open(out).read()


def _first_diff(a, b):
    al, bl = a.splitlines(), b.splitlines()
    for i in range(max(len(al), len(bl))):
        x = al[i] if i < len(al) else "<none>"
        y = bl[i] if i < len(bl) else "<none>"
        if x != y:
            return "row %d\n  %s\n  %s (%d vs %d rows)" % (i, x, y, len(al), len(bl))
    return None


CASES = [
    ("m", ["--cpg", "--ref", "{fa}", "--filter-threshold", "0.7"]),
    ("hm", ["--cpg", "--ref", "{fa}", "--combine-strands", "--no-filtering"]),
    ("hmf", ["--cpg", "--ref", "{fa}", "--filter-threshold", "0.6"]),                 # three codes: four ML requests and the base request
    ("h_m", ["--preset", "traditional", "--ref", "{fa}", "--filter-threshold", "0.6"]),
    ("hm", ["--preset", "traditional", "--ref", "{fa}", "--no-filtering"]),
    ("hmfc", ["--preset", "traditional", "--ref", "{fa}", "--no-filtering"]),          # three codes and the collapsed one: five ML requests
]


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_split_plane_fused_vs_events_vs_oracle(oracle_bin, tmp_path, ci):
    layout, flags = CASES[ci]
    bam_model = SplitPlaneBam(9100 + ci, layout)
    assert_not_vacuous(bam_model)
    bam, fa = bam_model.write(str(tmp_path / "sp"), index=ci % 2 == 0)   # indexed: device ingest
    flags = [f.format(fa=fa) for f in flags]
    ora = _oracle(oracle_bin, bam, str(tmp_path / "ora.bed"), flags)
    fused = _device(bam, str(tmp_path / "fused.bed"), flags, True)
    events = _device(bam, str(tmp_path / "events.bed"), flags, False)
    assert len(ora.splitlines()) > 500
    d = _first_diff(fused, ora)
    assert d is None, "fused decoder vs oracle: " + d
    d = _first_diff(events, ora)
    assert d is None, "event decoders vs oracle: " + d


@pytest.mark.parametrize("layout,flags", [("hmf", ["--cpg", "--filter-threshold", "0.7"]), ("h_m", ["--preset", "traditional", "--no-filtering"])])
def test_split_plane_relaunch_returns_first_pass(oracle_bin, tmp_path, layout, flags):
    bam_model = SplitPlaneBam(9301, layout)
    assert_not_vacuous(bam_model)
    bam, fa = bam_model.write(str(tmp_path / "sp"), index=True)
    flags = flags + ["--ref", fa]
    ora = _oracle(oracle_bin, bam, str(tmp_path / "ora.bed"), flags)
    want = modkit_amd.rows_digest(modkit_amd.read_bedmethyl(str(tmp_path / "ora.bed")))
    dev = str(tmp_path / "dev.bed")
    ctx = modkit_amd.Context(device=0)
    try:
        rep = ctx.pileup_run([bam, dev] + flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and open(dev).read() == ora
        one_shot = modkit_amd.rows_to_numpy(ctx.rerun(0, fetch=True))
        assert modkit_amd.rows_digest(one_shot) == want
        again = modkit_amd.rows_to_numpy(ctx.rerun(3, fetch=True))   # three re-launches on the resident shard (the planes are not rebuilt)
        assert modkit_amd.rows_digest(again) == want
    finally:
        ctx.close()
