"""Truth-table modBAMs for the threshold caller: every call of a layout at a reference position of its own, so that each bedMethyl
row holds one call and the call can be read back from N_mod / N_other_mod / N_canonical / N_fail (tests/caller_model.py predicts them).

The contig is "ACGT" repeated: every C is the first base of a CpG, so `--cpg` runs see every call.  Reads are exact matches of the
reference that tile it without overlapping.  A forward read's calls sit on the C of each unit (+ strand); a reverse read stores the
same bases, and its calls (the C's of the read's forward sequence) sit on the G of each unit (- strand), last call first.  Every C of a
read is listed (MM deltas of 0), so no call is inferred.

Layouts and the decode class each lands in (class_ids, mkp_plan.hpp; the layout is `fast` when all its tags have one base and
strand and no code repeats, mkp_pack.hpp:117-121):
    m        C+m?                 one explicit tag                   -> class 0 (SPARSE, one tag)
    hm       C+hm?                one explicit tag, two codes        -> class 0
    hmf      C+hmf?               three codes                        -> class 0
    hmfc     C+hmfc?              four codes (MKP_KMAX)              -> class 0
    h_m      C+h?;C+m?            two explicit tags, same positions  -> class 1 (SPARSE, two tags)
    m_dot    C+m.                 implicit mode                      -> class 2 (FAST, one tag)
    h_m_dot  C+h.;C+m.            implicit mode, two tags            -> class 3 (FAST, two tags)
    chebi    C+m?;C+21839?;C+h?   three tags, a ChEBI-numbered code  -> class 4 (general)
The fused slot decoder takes classes 0 and 1 (its integer caller, or its f32 walk for a collapse share over three codes); the event
decoders take the rest, and every class under MKP_FUSED=0.
"""
import itertools
import random
import struct

import numpy as np

import caller_model as model

from bamfuzz import aux_bc, aux_z, bam_header, bam_record, bgzf_write, write_bai

CTG = "truth"
UNIT = "ACGT"
MAX_CALLS_PER_READ = 1024

LAYOUTS = {
    # name: (tags as (codes, mode), decode class)
    "m": ([("m", "?")], 0),
    "hm": ([("hm", "?")], 0),
    "hmf": ([("hmf", "?")], 0),
    "hmfc": ([("hmfc", "?")], 0),
    "h_m": ([("h", "?"), ("m", "?")], 1),
    "m_dot": ([("m", ".")], 2),
    "h_m_dot": ([("h", "."), ("m", ".")], 3),
    "chebi": ([("m", "?"), ("21839", "?"), ("h", "?")], 4),
}


def layout_codes(name):
    """The codes of a layout, in tag order (a ChEBI code is one code)."""
    out = []
    for codes, _ in LAYOUTS[name][0]:
        out += [codes] if codes.isdigit() else list(codes)
    return out


def layout_tags(name):
    """[(code list of the tag, mode)]"""
    return [([codes] if codes.isdigit() else list(codes), mode) for codes, mode in LAYOUTS[name][0]]


def ml_content(name, seed=0):
    """The ML bytes of every call of a layout: (n, k) uint8, columns in layout_codes order, plus the rows that must sit in reads of
    their own (a pair whose sum fails combine_checked fails its whole read)."""
    r = random.Random(seed)
    k = len(layout_codes(name))
    if k == 1:
        return np.arange(256, dtype=np.uint8).reshape(-1, 1), np.zeros((0, 1), np.uint8)
    if name == "hm":
        h, m = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")   # all 65 536 pairs, sums above 1 included
        return np.stack([h.ravel(), m.ravel()], axis=1).astype(np.uint8), np.zeros((0, 2), np.uint8)
    if k == 2:   # two tags: (q_h + q_m + 1) / 256 > 1.01 fails, i.e. q_h + q_m >= 258
        pairs = [(h, m) for h in range(256) for m in range(256) if h + m <= 257]
        if name == "h_m_dot":
            pairs = [p for p in pairs if (p[0] * 7 + p[1] * 3) % 4 == 0 or p[0] + p[1] >= 250 or p[0] == p[1]]
        bad = [(h, s - h) for s in (258, 259, 260, 300, 510) for h in (s - 255, s // 2, 255) if 0 <= s - h <= 255][:12]
        return np.array(pairs, np.uint8), np.array(bad, np.uint8)
    rows = []
    special = [0, 1, 2, 63, 64, 85, 127, 128, 129, 170, 254, 255]
    for _ in range(3000):
        v = [r.choice(special) if r.random() < 0.4 else r.randrange(256) for _ in range(k)]
        if r.random() < 0.2:
            v[r.randrange(k)] = v[r.randrange(k)]                          # a tie between two codes
        rows.append(v)
    for a in special:                                                      # all codes equal
        rows.append([a] * k)
    arr = np.array(rows, np.uint8)
    if name == "chebi":   # several tags: keep the read (the sum in tag order must stay within 1.01)
        arr = arr[arr.astype(np.int64).sum(axis=1) + k <= 258]
        bad = np.array([[200, 100, 0], [0, 255, 10]], np.uint8)
        return arr, bad
    return arr, np.zeros((0, k), np.uint8)


class TruthBam:
    """Reads of one layout over the ML rows `ml` (n, k).  solo: rows that each go into a read of their own (after the others)."""

    def __init__(self, name, ml, solo=None, seed=0, reverse_share=0.5):
        self.name, self.ml = name, np.asarray(ml, np.uint8)
        self.solo = np.zeros((0, self.ml.shape[1]), np.uint8) if solo is None else np.asarray(solo, np.uint8)
        self.r = random.Random(seed)
        self.reverse_share = reverse_share
        # chunks: (first row, number of calls, solo?)
        chunks = []
        i, n = 0, len(self.ml)
        while i < n:
            c = min(n - i, self.r.choice([MAX_CALLS_PER_READ, 700, 333, 64, 1, 5]))
            chunks.append((i, c, False)); i += c
        chunks += [(j, 1, True) for j in range(len(self.solo))]
        self.chunks = chunks
        self.ctg_len = sum(4 * c + 8 for _, c, _ in chunks) + 64
        self.ref = (UNIT * (self.ctg_len // 4 + 1))[:self.ctg_len]

    def write(self, prefix, index=True):
        """Writes prefix.bam (+ .bai) and prefix.fa.  Returns (bam, fa, calls): calls = dict of arrays per call in row order of
        `ml` then `solo` (pos, strand '+'/'-', solo flag, read name, forward read position)."""
        tags = layout_tags(self.name)
        data = bam_header([(CTG, self.ctg_len)])
        idx, pos, strand, solo, rname, qpos = [], [], [], [], [], []
        at = 0
        for k, (first, c, is_solo) in enumerate(self.chunks):
            rows = (self.solo if is_solo else self.ml)[first:first + c]
            rev = self.r.random() < self.reverse_share
            L = 4 * c
            seq = self.ref[at:at + L]
            mm, ml = "", []
            col = 0
            for codes, mode in tags:
                mm += "C+%s%s%s;" % ("".join(codes), mode, ",0" * c)
                ncol = len(codes)
                ml += [int(v) for v in rows[:, col:col + ncol].ravel()]
                col += ncol
            name = "%s_%05d" % (self.name, k)
            rec = bam_record(0, at, 16 if rev else 0, name, [(L, "M")], seq, aux_z("MM", mm) + aux_bc("ML", ml))
            idx.append((0, at, L, 16 if rev else 0, len(data), len(rec)))
            data += rec
            for i in range(c):
                pos.append(at + (4 * (c - 1 - i) + 2 if rev else 4 * i + 1))
                strand.append("-" if rev else "+")
                solo.append(is_solo)
                rname.append(name)
                qpos.append(4 * i + 1)
            at += L + 8
        offs = bgzf_write(prefix + ".bam", bytes(data))
        if index:
            write_bai(prefix + ".bam.bai", 1, offs, idx)
        with open(prefix + ".fa", "w") as f:
            f.write(">%s\n" % CTG)
            for i in range(0, self.ctg_len, 60):
                f.write(self.ref[i:i + 60] + "\n")
        calls = dict(pos=np.array(pos, np.int64), strand=np.array(strand), solo=np.array(solo, bool), read=np.array(rname), qpos=np.array(qpos))
        return prefix + ".bam", prefix + ".fa", calls


# ---------------------------------------------------------------------------------------------------------------------------------
# expectations (tests/caller_model.py) and read-back

class Spec:
    """One caller configuration: default threshold (None: --no-filtering), per-base {base: t}, per-mod {code: t}, the --ignore code,
    --preset traditional.  flags() gives the command line, thresholds as the shortest repr of their f32."""

    def __init__(self, default=None, per_base=None, per_mod=None, ignore=None, traditional=False):
        self.default, self.per_base, self.per_mod = default, dict(per_base or {}), dict(per_mod or {})
        self.ignore = "h" if traditional else ignore
        self.traditional = traditional

    def flags(self):
        out = ["--no-filtering"] if self.default is None and not self.per_base and not self.per_mod else []
        if self.default is not None:
            out += ["--filter-threshold", model.shortest(self.default)]
        for b, t in self.per_base.items():
            out += ["--filter-threshold", "%s:%s" % (b, model.shortest(t))]
        for c, t in self.per_mod.items():
            out += ["--mod-thresholds", "%s:%s" % (c, model.shortest(t))]
        if self.traditional:
            out += ["--preset", "traditional"]
        elif self.ignore:
            out += ["--ignore", self.ignore]
        return out

    def __repr__(self):
        return " ".join(self.flags())


def expected_calls(name, ml, solo, calls, spec):
    """Per call (rows of ml, then solo): the threshold call ('F' filtered, '-' canonical, or the code), the argmax call ('-' or the
    code), its probability (f32), whether the read fails combine_checked, and whether the answer depends on the map's iteration order.
    Returns a dict of arrays."""
    codes = layout_codes(name)
    allq = np.concatenate([ml, solo]).astype(np.int64)
    P = model.quals_to_probs(allq)
    # combine_checked over the tags, under every iteration order (they must agree: sums of multiples of 2^-9 are exact)
    tags = layout_tags(name)
    col, tag_probs = 0, []
    for tc, _ in tags:
        tag_probs.append(([codes.index(c) for c in tc], P[:, col:col + len(tc)])); col += len(tc)
    fails = None
    for order in itertools.permutations(range(len(codes))):
        f = model.combine_fails(tag_probs, list(order))
        assert fails is None or (f == fails).all()
        fails = f
    read_fail = {r for r, f in zip(calls["read"], fails) if f}
    failed = np.array([r in read_fail for r in calls["read"]], bool)
    default = 0.0 if spec.default is None else spec.default
    ev = model.evaluate(codes, P, base="C", default=default, per_base=spec.per_base, per_mod=spec.per_mod, collapse=spec.ignore)

    def name_of(c):
        return np.array(["F" if x == model.FILTERED else "-" if x == model.CANONICAL else codes[x] for x in c])
    return dict(cls=name_of(ev["cls"]), argmax=name_of(ev["argmax_cls"]), argmax_p=ev["argmax_p"], failed=failed, order_dep=ev["order_dep"],
                n_out_codes=len(ev["out_codes"]))


def bed_calls(path, calls, combine=False):
    """The call at each call position read back from a bedMethyl file: '.' no row (filtered, or the read failed), '-' canonical,
    or the code of the row with N_mod = 1.  Raises when a position holds anything but one call."""
    at = {}
    for ln in open(path):
        f = ln.rstrip("\n").split("\t") if "\t" in ln else ln.split()
        pos, code, strand = int(f[1]), f[3], f[5]
        n_valid, n_mod, n_can, n_other, n_fail = int(f[9]), int(f[11]), int(f[12]), int(f[13]), int(f[15])
        key = pos if combine else (pos, strand)
        assert n_valid == 1 and n_fail == 0 and n_mod + n_can + n_other == 1, "row holds more than one call: " + ln
        got = "-" if n_can else code if n_mod else None
        prev = at.get(key)
        if got is not None:
            assert prev in (None, got), "two calls at " + ln
            at[key] = got
        else:
            at.setdefault(key, None)
    out = []
    for p, s in zip(calls["pos"], calls["strand"]):
        key = (p - 1 if s == "-" else p) if combine else (p, s)
        v = at.get(key, ".")
        out.append("?" if v is None else v)   # '?': rows whose calls are all other-mod (a code without a row of its own)
    return np.array(out)


def expected_bed(exp):
    """What bed_calls should read for each call (a map left without codes by the collapse has no row to count in)."""
    return np.where(exp["failed"] | (exp["cls"] == "F") | (exp["n_out_codes"] == 0), ".", exp["cls"])


def first_mismatch(what, got, want, skip, name, ml, solo, calls, spec):
    """None, or a report of the first call where got != want (order-dependent calls skipped): position, ML bytes, flags, both answers."""
    bad = np.nonzero((got != want) & ~skip)[0]
    if not len(bad):
        return None
    i = int(bad[0])
    allq = np.concatenate([ml, solo])
    return "%s: %d of %d calls differ; first at %s%s (read %s), layout %s ML %s, flags %s: got %r, model %r" % (
        what, len(bad), len(got), calls["pos"][i], calls["strand"][i], calls["read"][i], name, list(allq[i]), spec, got[i], want[i])


def extract_rows(path):
    """`extract calls` rows: {(read, forward position): (call_prob text, call_code, fail)}"""
    out = {}
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        ix = {k: head.index(k) for k in ("read_id", "forward_read_position", "call_prob", "call_code", "fail")}
        for ln in f:
            c = ln.rstrip("\n").split("\t")
            out[(c[ix["read_id"]], int(c[ix["forward_read_position"]]))] = (c[ix["call_prob"]], c[ix["call_code"]], c[ix["fail"]])
    return out


def check_extract(path, name, ml, solo, calls, spec, oracle_path=None):
    """None or the first disagreement of an `extract calls` table with the model (order-dependent calls: with the oracle's table)."""
    exp = expected_calls(name, ml, solo, calls, spec)
    rows = extract_rows(path)
    ora = extract_rows(oracle_path) if oracle_path else None
    allq = np.concatenate([ml, solo])
    for i in range(len(calls["pos"])):
        key = (calls["read"][i], int(calls["qpos"][i]))
        got = rows.get(key)
        if exp["failed"][i] or exp["n_out_codes"] == 0:   # (a map left without codes by the collapse has no call to list)
            want = None
        elif exp["order_dep"][i]:
            if ora is None:
                continue
            want = ora.get(key)
        else:
            want = (model.shortest(exp["argmax_p"][i]), exp["argmax"][i], "true" if exp["cls"][i] == "F" else "false")
        if got != want:
            return "extract calls: first disagreement at %s%s (read %s, position %d), layout %s ML %s, flags %s: got %r, %s %r" % (
                calls["pos"][i], calls["strand"][i], key[0], key[1], name, list(allq[i]), spec, got,
                "oracle" if exp["order_dep"][i] else "model", want)
    n_fail_reads = len({r for r, f in zip(calls["read"], exp["failed"]) if f})
    n_want = int((~exp["failed"]).sum()) if exp["n_out_codes"] else 0
    if len(rows) != n_want:
        return "extract calls: %d rows, model %d (%d failed reads)" % (len(rows), n_want, n_fail_reads)
    return None


def threshold_specs(name, qs=(0, 1, 127, 128, 254, 255)):
    """--filter-threshold at p(q) and one f32 ulp either side of it"""
    out = []
    for q in qs:
        p = model.quals_to_probs(q)
        for t in (p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(2))):
            out.append(Spec(default=np.float32(t)))
    return out


def share_value(qx, qo, n_other):
    """p(qo) + p(qx) / n_other in f32: a collapsed entry's probability (ReDistribute)"""
    px, po = model.quals_to_probs(qx), model.quals_to_probs(qo)
    return np.float32(po + np.float32(px / np.float32(n_other)))


def specs_for(name):
    """The caller configurations a layout runs under (a bounded set: the threshold sweep is spread over the layouts)."""
    codes = layout_codes(name)
    k = len(codes)
    s = [Spec(), Spec(default=0.0), Spec(default=1.5), Spec(default=0.6, per_base={"C": 0.75})]
    sweep = {"m": (0, 1, 127, 128, 254, 255), "m_dot": (0, 128, 255), "hm": (1, 127, 254), "h_m": (0, 128, 255),
             "h_m_dot": (127,), "hmf": (64,), "hmfc": (85,), "chebi": (128,)}[name]
    s += threshold_specs(name, sweep)
    if k >= 2:
        s += [Spec(default=0.3, per_mod={"h": 0.8}), Spec(default=0.7, per_mod={"m": 0.55}), Spec(default=0.9, per_mod={"C": 0.6, "m": 0.8})]
    if "h" in codes:
        n_other = k   # ignore h: the other codes and canonical share it
        t = share_value(100, 50, n_other)
        s += [Spec(ignore="h"), Spec(default=0.6, ignore="h")]
        s += [Spec(default=np.float32(x), ignore="h") for x in (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(2)))]
        s += [Spec(default=0.55, traditional=True)]
    if "m" in codes:
        s += [Spec(default=0.5, ignore="m")]
    if k >= 3:
        for c in codes[2:]:
            s += [Spec(default=0.4, ignore=c)]
    return s


def expected_summary(exp):
    """`modkit summary` counts of the calls (summarize.rs): a passing call counts as pass under its thresholded class, a filtered one as
    fail under its argmax class.  {(base, code or '-'): (pass, fail)} without the rows that count nothing."""
    out = {}
    live = ~exp["failed"] & (exp["n_out_codes"] > 0)
    for c, a in zip(exp["cls"][live], exp["argmax"][live]):
        key = ("C", a if c == "F" else c)
        p, f = out.get(key, (0, 0))
        out[key] = (p, f + 1) if c == "F" else (p + 1, f)
    return out


def summary_rows(s):
    return {k: v for k, v in s["rows"].items() if v != (0, 0)}


# layouts and configurations whose summary no iteration order can change (so the model decides every count)
SUMMARY_CASES = [("m", Spec(default=0.6)), ("m", Spec(default=float(model.quals_to_probs(128)))), ("m_dot", Spec(per_base={"C": 0.7})),
                 ("hm", Spec(default=0.6, ignore="h")), ("h_m", Spec(default=0.7, ignore="m")), ("m", Spec())]


def argmax_sample(exp):
    """The sorted f32 sample threshold estimation sees: argmax_base_mod_call's probability of every call that reaches it."""
    live = ~exp["failed"] & (exp["n_out_codes"] > 0)
    return np.sort(exp["argmax_p"][live])
