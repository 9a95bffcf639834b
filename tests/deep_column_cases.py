"""Piles deeper than 65 535 records over one column (the wide-tally kernels).  Records are built from a handful of templates
(bamfuzz.bam_record) that differ only in their fixed-width names, so that a pile of 70 000 reads is written in a second or two."""
import random

from bamfuzz import aux_bc, aux_i, aux_z, bam_header, bam_record, bgzf_write, revcomp, write_bai

NAME = "r%07d"   # fixed width: a template's name bytes are overwritten in place
NAME_AT = 4 + 32  # block_size + the fixed fields in front of read_name


def reference(length, seed=11):
    """A contig with a CpG every ~12 bases and no run that hides the C calls of a read."""
    r = random.Random(seed)
    s = []
    while len(s) < length:
        s.extend(r.choice("ACGT") for _ in range(r.randint(6, 16)))
        s.extend("CG")
    return "".join(s[:length])


def write_fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(seq), 60):
            f.write(seq[i:i + 60] + "\n")
    return path


def _mods(seq, rev, kind, ml):
    """MM/ML of calls on the read's first twelve Cs (read orientation), ML values cycling through `ml`: kind 'm' = C+m?, 'hm' = C+hm?."""
    n_c = (revcomp(seq) if rev else seq).count("C")
    k = min(12, n_c)
    mm = "C+%s?%s;" % (kind, ",0" * k)
    return aux_z("MM", mm) + aux_bc("ML", (ml * (k * len(kind)))[:k * len(kind)])


class Template:
    """One record shape at one start: CIGAR, SEQ (the reference's bases) and tags; records differ only in their names."""

    def __init__(self, ref, rel, cigar, rev, kind, ml, key=None):
        seq, r = [], rel
        for ln, op in cigar:
            if op == "M":
                seq.append(ref[r:r + ln]); r += ln
            elif op in "DN":
                r += ln
        seq = "".join(seq)
        aux = _mods(seq, rev, kind, ml) + (aux_i("HP", key) if key is not None else b"")
        self.rel, self.span = rel, r - rel
        self.base = bam_record(0, rel, 16 if rev else 0, NAME % 0, cigar, seq, aux)

    def record(self, k):
        """(start, span, the record named k)"""
        rec = bytearray(self.base)
        rec[NAME_AT:NAME_AT + 8] = (NAME % k).encode()
        return self.rel, self.span, bytes(rec)


def write_bam(prefix, contig, recs, index=False):
    """recs: (pos, span, record bytes), any order -> coordinate-sorted BAM (+ BAI)."""
    recs = sorted(recs, key=lambda x: x[0])
    data = bytearray(bam_header([contig]))
    idx = []
    for pos, span, rec in recs:
        idx.append((0, pos, span, 0, len(data), len(rec)))
        data.extend(rec)
    offs = bgzf_write(prefix + ".bam", bytes(data))
    if index:
        write_bai(prefix + ".bam.bai", 1, offs, idx)
    return prefix + ".bam"


def amplicon_key(k, n_fwd):
    """HP key of the k-th amplicon read: 2 on every 32nd forward read, 1 on the others and on every reverse read (both strands of key 1
    deeper than 65 535 on the '+' tallies of a 70 000-read pile)"""
    return 2 if k < n_fwd and k % 32 == 31 else 1


def amplicon_records(ref, at, n_fwd, n_rev, length=300, keys=False, first=0):
    """n_fwd forward and n_rev reverse reads over [at, at + length): C+m? on most, C+hm? on every fourth, a deletion on every 53rd and a
    ref-skip on every 71st; ML values that give modified, canonical and filtered calls at a 0.7 threshold.  keys: an HP:i tag
    (amplicon_key).  -> [(pos, span, bytes)], names first, first + 1, ..."""
    mls = [[250, 250, 250], [10, 20, 5], [140, 230, 15]]
    mls_hm = [[200, 30, 20, 10, 120, 120], [10, 240, 5, 5, 250, 2]]
    cache = {}
    out = []
    for k in range(n_fwd + n_rev):
        rev = k >= n_fwd
        key = amplicon_key(k, n_fwd) if keys else None
        if k % 71 == 5:
            shape = ("N", rev, key, k % 2)
        elif k % 53 == 7:
            shape = ("D", rev, key, k % 2)
        elif k % 4 == 3:
            shape = ("hm", rev, key, k % 2)
        else:
            shape = ("m", rev, key, k % 3)
        t = cache.get(shape)
        if t is None:
            kind, _, _, v = shape
            if kind == "N":
                cig = [(100, "M"), (40, "N"), (length - 100, "M")]
            elif kind == "D":
                cig = [(120, "M"), (4, "D"), (length - 124, "M")]
            else:
                cig = [(length, "M")]
            if kind == "hm":
                t = Template(ref, at, cig, rev, "hm", mls_hm[v], key)
            else:
                t = Template(ref, at, cig, rev, "m", mls[v % 3], key)
            cache[shape] = t
        out.append(t.record(first + k))
    return out


def background_records(ref, contig_len, depth, length=300, seed=5, first=0):
    """~depth x coverage of forward / reverse reads at random starts (C+m?), names first, first + 1, ..."""
    r = random.Random(seed)
    out = []
    n = contig_len * depth // length
    for k in range(n):
        pos = r.randrange(0, contig_len - length)
        t = Template(ref, pos, [(length, "M")], r.random() < 0.5, "m", [r.choice([250, 10, 140])] * 3)
        out.append(t.record(first + k))
    return out


def stack_records(ref, at, n, length=60):
    """n forward reads over [at, at + length): C+m? calls, one pile of exactly n records over every column of it."""
    t = Template(ref, at, [(length, "M")], False, "m", [250, 10, 250])
    return [t.record(k) for k in range(n)]
