"""GPU parity of the slot decoder's call plane (mkp_call_plane: per fused read, one bit per stored base "a listed call sits here" and the
listed calls before every 32 bases, built once when the shard becomes resident).  Seeded modBAMs whose reads sit on the plane's edges —
lengths around a plane word (31/32/33/63/64/65), around the former 13 312-base window, over 65 536 bases; reverse reads; odd lengths whose
pad nibble equals the counted base; N bases; tags without calls; delta lists that run past the base's last occurrence; `C+hm?`,
`C+h?;C+m?` and `A+a?` — run through the fused decoder, through the event decoders (MKP_FUSED=0) and through the oracle: the three
bedMethyl files must be equal byte for byte.  A re-launch on the resident shard must give back the first pass's rows."""
import os
import random
import struct

import pytest

import modkit_amd
from bamfuzz import NT16, aux_bc, aux_z, bam_header, bgzf_write, revcomp, write_bai

pytestmark = pytest.mark.gpu

CTG = "plane"
CTG_LEN = 160_000
EDGE_LENGTHS = [31, 32, 33, 63, 64, 65, 13_311, 13_312, 13_313, 70_001, 66_000]


def _record(tid, pos, flag, qname, cigar, seq, aux, pad_code):
    qn = qname.encode() + b"\0"
    cg = b"".join(struct.pack("<I", (n << 4) | "MIDNSHP=X".index(op)) for n, op in cigar)
    sq = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        sq[i // 2] |= NT16[c] << (4 if i % 2 == 0 else 0)
    if len(seq) % 2:
        sq[-1] |= pad_code   # the low nibble of the last byte is not a base
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qn), 60, 4680, len(cigar), flag, len(seq), -1, -1, 0) + qn + cg + bytes(sq) \
        + b"\xff" * len(seq) + aux
    return struct.pack("<i", len(body)) + body


class PlaneBam:
    """profile: "hm_comb" (C+hm?), "hm_split" (C+h?;C+m?), "m" (C+m?), "a" (A+a?)"""

    def __init__(self, seed, profile, n_random=300):
        self.r = random.Random(seed)
        self.profile = profile
        s = [self.r.choice("ACGT") for _ in range(CTG_LEN)]
        for _ in range(CTG_LEN // 30):
            p = self.r.randrange(CTG_LEN - 1)
            s[p], s[p + 1] = "C", "G"
        self.ref = "".join(s)
        self.lengths = EDGE_LENGTHS * 2 + [self.r.choice([self.r.randrange(20, 400), self.r.randrange(400, 9000)]) for _ in range(n_random)]

    def _read(self, qlen):
        r, ref = self.r, self.ref
        ops, seq = [], []
        sc = r.randrange(0, 12) if qlen > 100 else 0
        if sc:
            ops.append((sc, "S")); seq += [r.choice("ACGT") for _ in range(sc)]
        start = r.randrange(0, CTG_LEN - qlen - qlen // 5 - 100)
        rp = start
        while len(seq) < qlen:
            left = qlen - len(seq)
            x = r.random()
            if x < 0.05 and ops and ops[-1][1] == "M" and left > 1:
                n = min(left - 1, r.randrange(1, 6)); ops.append((n, "I")); seq += [r.choice("ACGT") for _ in range(n)]
            elif x < 0.10 and ops and ops[-1][1] == "M":
                n = r.randrange(1, 6); ops.append((n, "D")); rp += n
            else:
                n = min(left, r.randrange(1, 300))
                for k in range(n):
                    b = ref[rp + k]
                    y = r.random()
                    seq.append("N" if y < 0.01 else r.choice("ACGT") if y < 0.03 else b)
                ops.append((n, "M")); rp += n
        return start, ops, "".join(seq)

    def _tags(self, fwd):
        r = self.r
        base = "A" if self.profile == "a" else "C"
        occ = [i for i, c in enumerate(fwd) if c == base]
        kind = r.random()
        if kind < 0.06 or not occ:
            picked = []                                              # a tag without calls
        else:
            dens = r.choice([1.0, 0.5, 0.05])
            picked = [i for i in range(len(occ)) if r.random() < dens]
        deltas, prev = [], -1
        for i in picked:
            deltas.append(i - prev - 1); prev = i
        if deltas and kind > 0.94:
            deltas.append(len(occ) - prev + r.randrange(0, 3))        # runs past the base's last occurrence
        n = len(deltas)
        lst = "".join("," + str(d) for d in deltas)

        def probs(k):
            out = []
            for _ in range(k):
                v = r.choice([r.randrange(256), 0, 255, 128, 200, 50])
                out.append(v)
            return out
        if self.profile == "a":
            return aux_z("MM", "A+a?%s;" % lst) + aux_bc("ML", probs(n))
        if self.profile == "m":
            return aux_z("MM", "C+m?%s;" % lst) + aux_bc("ML", probs(n))
        hs, ms = [], []
        for _ in range(n):   # (h + m above 1.01 fails the record: combine_checked, a test of its own elsewhere)
            h = r.choice([r.randrange(0, 200), 0, 128]); hs.append(h); ms.append(r.choice([r.randrange(0, 256 - h), 255 - h, 0]))
        if self.profile == "hm_comb":
            return aux_z("MM", "C+hm?%s;" % lst) + aux_bc("ML", [v for hm in zip(hs, ms) for v in hm])
        return aux_z("MM", "C+h?%s;C+m?%s;" % (lst, lst)) + aux_bc("ML", hs + ms)

    def write(self, prefix, index):
        data = bam_header([(CTG, CTG_LEN)])
        base = "A" if self.profile == "a" else "C"
        recs = []
        for k, qlen in enumerate(self.lengths):
            start, ops, seq = self._read(qlen)
            rev = self.r.random() < 0.5
            fwd = revcomp(seq) if rev else seq
            stored = {"A": "T", "C": "G"}[base] if rev else base
            pad = NT16[stored] if self.r.random() < 0.7 else 0
            recs.append((start, 16 if rev else 0, ops, seq, self._tags(fwd), pad, "r%05d" % k))
        recs.sort(key=lambda t: t[0])
        idx = []
        for start, flag, ops, seq, aux, pad, name in recs:
            rec = _record(0, start, flag, name, ops, seq, aux, pad)
            idx.append((0, start, sum(n for n, op in ops if op in "MDN=X"), flag, len(data), len(rec)))
            data += rec
        offs = bgzf_write(prefix + ".bam", bytes(data))
        if index:
            write_bai(prefix + ".bam.bai", 1, offs, idx)
        with open(prefix + ".fa", "w") as f:
            f.write(">%s\n" % CTG)
            for i in range(0, CTG_LEN, 60):
                f.write(self.ref[i:i + 60] + "\n")
        return prefix + ".bam", prefix + ".fa"


def _oracle(oracle_bin, bam, out, flags):
    import subprocess
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
    ("hm_comb", ["--cpg", "--ref", "{fa}", "--filter-threshold", "0.7"]),
    ("hm_comb", ["--cpg", "--ref", "{fa}", "--combine-strands", "--no-filtering"]),
    ("hm_comb", ["--cpg", "--ref", "{fa}", "--ignore", "h", "--filter-threshold", "0.66"]),
    ("hm_split", ["--cpg", "--ref", "{fa}", "--filter-threshold", "0.75"]),
    ("hm_split", ["--motif", "CG", "0", "--ref", "{fa}", "--ignore", "h", "--no-filtering"]),
    ("m", ["--cpg", "--ref", "{fa}", "--combine-strands", "--filter-threshold", "0.6"]),
    ("a", ["--motif", "A", "0", "--ref", "{fa}", "--no-filtering"]),
    ("a", ["--motif", "A", "0", "--ref", "{fa}", "--filter-threshold", "0.7"]),
]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_call_plane_fused_vs_events_vs_oracle(oracle_bin, tmp_path, ci, seed):
    profile, flags = CASES[ci]
    bam, fa = PlaneBam(7100 + 10 * ci + seed, profile).write(str(tmp_path / "pl"), index=seed == 0)   # indexed: device ingest
    flags = [f.format(fa=fa) for f in flags]
    ora = _oracle(oracle_bin, bam, str(tmp_path / "ora.bed"), flags)
    fused = _device(bam, str(tmp_path / "fused.bed"), flags, True)
    events = _device(bam, str(tmp_path / "events.bed"), flags, False)
    assert len(ora.splitlines()) > 1000
    d = _first_diff(fused, ora)
    assert d is None, "fused decoder vs oracle: " + d
    d = _first_diff(events, ora)
    assert d is None, "event decoders vs oracle: " + d


def test_call_plane_relaunch_returns_first_pass(oracle_bin, tmp_path):
    bam, fa = PlaneBam(7301, "hm_split").write(str(tmp_path / "pl"), index=True)
    flags = ["--cpg", "--ref", fa, "--filter-threshold", "0.7"]
    ora = _oracle(oracle_bin, bam, str(tmp_path / "ora.bed"), flags)
    want = modkit_amd.rows_digest(modkit_amd.read_bedmethyl(str(tmp_path / "ora.bed")))
    dev = str(tmp_path / "dev.bed")
    ctx = modkit_amd.Context(device=0)
    try:
        rep = ctx.pileup_run([bam, dev] + flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and open(dev).read() == ora
        one_shot = modkit_amd.rows_to_numpy(ctx.rerun(0, fetch=True))
        assert modkit_amd.rows_digest(one_shot) == want
        again = modkit_amd.rows_to_numpy(ctx.rerun(3, fetch=True))   # three re-launches on the resident shard (the plane is not rebuilt)
        assert modkit_amd.rows_digest(again) == want
    finally:
        ctx.close()
