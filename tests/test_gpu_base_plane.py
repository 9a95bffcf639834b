"""GPU parity of the slot decoder's base-and-call plane (mkp_call_plane writes the 2-bit base of every stored base of every fused read
beside the call bits; mkp_decode_slots takes the base under a slot from it and reads the SEQ only for a read that holds a base that is not
A/C/G/T, MKP_RF_SEQN).  Seeded modBAMs that mix, in one shard: reads with N and other IUPAC codes on CpG positions (the SEQN path, whose
coverage features must see the real base), reads with mismatches on CpG positions (the base of a NoCall feature comes from the plane),
reads without tags, with a tag without calls and with a delta list that runs past its base (bases only, no calls), reverse reads,
lengths around one and two plane words, odd lengths, and reads over 8 192 bases (mostly SEQN reads with calls) — run through the
fused decoder, the event decoders (MKP_FUSED=0) and the oracle under --cpg and --preset traditional: the three bedMethyl files must be equal byte for byte, and a re-launch on the resident shard must
give back the first pass's rows."""
import os
import random
import subprocess

import pytest

import modkit_amd
from bamfuzz import NT16, aux_bc, aux_z, bam_header, bam_record, bgzf_write, write_bai

pytestmark = pytest.mark.gpu

CTG = "bplane"
CTG_LEN = 60_000
LENGTHS = [1, 2, 7, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 129]
# reads over 8 192 bases (256 plane words): the builder's path that loads the SEQ again for its second pass; most of them SEQN reads
LONG = [8191, 8192, 8193, 9000, 12345, 16384, 16385, 20000]
IUPAC = "NRYMKSWBDHV="
COMP = dict(zip("ACGTNRYMKSWBDHV=", "TGCANYRKMSWVHDB="))


def _revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


class BasePlaneBam:
    """profile: "m" (C+m?), "hm_comb" (C+hm?), "hm_split" (C+h?;C+m?)"""

    def __init__(self, seed, profile, n_random=500):
        self.r = random.Random(seed)
        self.profile = profile
        s = [self.r.choice("ACGT") for _ in range(CTG_LEN)]
        for _ in range(CTG_LEN // 25):
            p = self.r.randrange(CTG_LEN - 1)
            s[p], s[p + 1] = "C", "G"
        self.ref = "".join(s)
        self.cpg = {i for i in range(CTG_LEN - 1) if self.ref[i] == "C" and self.ref[i + 1] == "G"}
        self.cpg |= {i + 1 for i in self.cpg}
        self.lengths = LENGTHS * 6 + LONG * 2 + [self.r.choice([self.r.randrange(20, 300), self.r.randrange(300, 3000)]) for _ in range(n_random)]

    def _read(self, qlen, kind):
        """kind: "clean" (ACGT, reference bases), "seqn" (non-ACGT codes, many of them on CpG positions), "mismatch" (other ACGT bases on
        CpG positions)"""
        r, ref = self.r, self.ref
        ops, seq = [], []
        sc = r.randrange(0, 6) if qlen > 40 else 0
        if sc:
            ops.append((sc, "S")); seq += [r.choice("ACGT") for _ in range(sc)]
        start = r.randrange(0, CTG_LEN - qlen - qlen // 5 - 50)
        rp = start
        while len(seq) < qlen:
            left = qlen - len(seq)
            x = r.random()
            if x < 0.05 and ops and ops[-1][1] == "M" and left > 1:
                n = min(left - 1, r.randrange(1, 4)); ops.append((n, "I")); seq += [r.choice("ACGT") for _ in range(n)]
            elif x < 0.10 and ops and ops[-1][1] == "M":
                n = r.randrange(1, 4); ops.append((n, "D")); rp += n
            else:
                n = min(left, r.randrange(1, 120))
                for k in range(n):
                    b, focus = ref[rp + k], (rp + k) in self.cpg
                    y = r.random()
                    if kind == "seqn" and (y < (0.3 if focus else 0.02)):
                        b = r.choice(IUPAC)
                    elif kind == "mismatch" and focus and y < 0.4:
                        b = r.choice([c for c in "ACGT" if c != b])
                    seq.append(b)
                ops.append((n, "M")); rp += n
        return start, ops, "".join(seq)

    def _tags(self, fwd, tags):
        """tags: "calls", "none" (no MM / ML), "empty" (a tag without calls), "runover" (the delta list runs past the last C)"""
        r = self.r
        if tags == "none":
            return b""
        occ = [i for i, c in enumerate(fwd) if c == "C"]
        picked = [] if tags == "empty" or not occ else [i for i in range(len(occ)) if r.random() < r.choice([1.0, 0.5])]
        deltas, prev = [], -1
        for i in picked:
            deltas.append(i - prev - 1); prev = i
        if tags == "runover" and occ:
            deltas.append(len(occ) - prev + r.randrange(0, 3))
        n = len(deltas)
        lst = "".join("," + str(d) for d in deltas)
        if self.profile == "m":
            return aux_z("MM", "C+m?%s;" % lst) + aux_bc("ML", [r.choice([r.randrange(256), 0, 255, 200]) for _ in range(n)])
        hs, ms = [], []
        for _ in range(n):
            h = r.choice([r.randrange(0, 200), 0, 128]); hs.append(h); ms.append(r.choice([r.randrange(0, 256 - h), 255 - h, 0]))
        if self.profile == "hm_comb":
            return aux_z("MM", "C+hm?%s;" % lst) + aux_bc("ML", [v for hm in zip(hs, ms) for v in hm])
        return aux_z("MM", "C+h?%s;C+m?%s;" % (lst, lst)) + aux_bc("ML", hs + ms)

    def write(self, prefix, index):
        data = bam_header([(CTG, CTG_LEN)])
        recs = []
        for k, qlen in enumerate(self.lengths):
            if qlen > 8192:
                kind = self.r.choice(["seqn", "seqn", "seqn", "clean"])
                tags = self.r.choice(["calls"] * 5 + ["runover"])
            else:
                kind = self.r.choice(["clean", "clean", "seqn", "mismatch"])
                tags = self.r.choice(["calls"] * 7 + ["none", "empty", "runover"])
            start, ops, seq = self._read(qlen, kind)
            rev = self.r.random() < 0.5
            fwd = _revcomp(seq) if rev else seq
            recs.append((start, 16 if rev else 0, ops, seq, self._tags(fwd, tags), "r%05d" % k))
        recs.sort(key=lambda t: t[0])
        idx = []
        for start, flag, ops, seq, aux, name in recs:
            rec = bam_record(0, start, flag, name, ops, seq, aux)
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
    ("hm_comb", ["--cpg", "--ref", "{fa}", "--combine-strands", "--no-filtering"]),
    ("hm_split", ["--preset", "traditional", "--ref", "{fa}", "--filter-threshold", "0.6"]),
    ("hm_comb", ["--preset", "traditional", "--ref", "{fa}", "--no-filtering"]),
]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_base_plane_fused_vs_events_vs_oracle(oracle_bin, tmp_path, ci, seed):
    profile, flags = CASES[ci]
    bam, fa = BasePlaneBam(8100 + 10 * ci + seed, profile).write(str(tmp_path / "bp"), index=seed == 0)   # indexed: device ingest
    flags = [f.format(fa=fa) for f in flags]
    ora = _oracle(oracle_bin, bam, str(tmp_path / "ora.bed"), flags)
    fused = _device(bam, str(tmp_path / "fused.bed"), flags, True)
    events = _device(bam, str(tmp_path / "events.bed"), flags, False)
    assert len(ora.splitlines()) > 1000
    d = _first_diff(fused, ora)
    assert d is None, "fused decoder vs oracle: " + d
    d = _first_diff(events, ora)
    assert d is None, "event decoders vs oracle: " + d


@pytest.mark.parametrize("profile,flags", [("hm_split", ["--cpg", "--filter-threshold", "0.7"]), ("m", ["--preset", "traditional", "--no-filtering"])])
def test_base_plane_relaunch_returns_first_pass(oracle_bin, tmp_path, profile, flags):
    bam, fa = BasePlaneBam(8301, profile).write(str(tmp_path / "bp"), index=True)
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
        again = modkit_amd.rows_to_numpy(ctx.rerun(3, fetch=True))   # three re-launches on the resident shard (the plane is not rebuilt)
        assert modkit_amd.rows_digest(again) == want
    finally:
        ctx.close()
