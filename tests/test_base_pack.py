"""The base half of the slot decoder's plane: mkp_pack_bases8 / mkp_pack_bases32 (modkit_amd/csrc/mkp_base_pack.hpp, what
mkp_call_plane writes per 32 stored bases) and mkp_bases_eq (the builder's flag bitmap of the counted base, taken from the codes) compiled
for the host with g++ and run on random SEQ dwords, against a numpy model of the BAM nibble order (base 2j = high nibble of byte j), the
2-bit codes (A=0 C=1 G=2 T=3) and the not-A/C/G/T flags — odd lengths, the pad nibble and tails past the read's end, N and the other
IUPAC codes included."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "mkp_base_pack.hpp"
#include <cstdio>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  uint32_t r[5];
  while (fread(r, 4, 5, f) == 5) {   // four SEQ dwords + the bases of the word that belong to the read
    uint32_t lo = 0, hi = 0;
    const uint32_t bad = mkp_pack_bases32(r[0], r[1], r[2], r[3], r[4], &lo, &hi);
    const uint32_t p8 = mkp_pack_bases8(r[0], r[4] < 8u ? r[4] : 8u);
    const uint32_t out[8] = {lo, hi, bad, p8, mkp_bases_eq(lo, hi, 0), mkp_bases_eq(lo, hi, 1), mkp_bases_eq(lo, hi, 2), mkp_bases_eq(lo, hi, 3)};
    fwrite(out, 4, 8, o);
  }
  fclose(f); fclose(o); return 0;
}
"""


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    d = tmp_path_factory.mktemp("base_pack")
    src, exe = d / "pack.cpp", d / "pack"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "modkit_amd", "csrc"), "-o", str(exe), str(src)])

    def run(words, n_valid):
        inp, out = d / "in.bin", d / "out.bin"
        np.concatenate([words.astype("<u4"), n_valid.astype("<u4")[:, None]], axis=1).tofile(inp)
        subprocess.check_call([str(exe), str(inp), str(out)])
        return np.fromfile(out, dtype="<u4").reshape(-1, 8)
    return run


def model(words, n_valid):
    """lo, hi, bad flags, the first dword's 8-base packing and the eq bitmaps of codes 0..3, base by base"""
    n = len(words)
    by = words.astype("<u4").view(np.uint8).reshape(n, 16)        # the word's 16 SEQ bytes in memory order
    nib = np.empty((n, 32), dtype=np.uint32)
    nib[:, 0::2] = by >> 4                                          # base 2j: high nibble of byte j
    nib[:, 1::2] = by & 15
    one_hot = {1: 0, 2: 1, 4: 2, 8: 3}
    code = np.vectorize(lambda x: one_hot.get(int(x), 0), otypes=[np.uint32])(nib)
    is_acgt = np.isin(nib, list(one_hot))
    inread = np.arange(32)[None, :] < n_valid[:, None]
    code = np.where(is_acgt & inread, code, 0).astype(np.uint64)
    bad = (~is_acgt & inread).astype(np.uint64)
    sh2 = (2 * np.arange(16)).astype(np.uint64)
    lo = (code[:, :16] << sh2).sum(axis=1)
    hi = (code[:, 16:] << sh2).sum(axis=1)
    badw = (bad << np.arange(32).astype(np.uint64)).sum(axis=1)
    p8 = (code[:, :8] << sh2[:8]).sum(axis=1) | ((bad[:, :8] << np.arange(8).astype(np.uint64)).sum(axis=1) << np.uint64(16))
    eq = [((code == k).astype(np.uint64) << np.arange(32).astype(np.uint64)).sum(axis=1) for k in range(4)]   # of the packed codes
    return np.stack([lo, hi, badw, p8] + eq, axis=1).astype(np.uint32)


ACGT = np.array([1, 2, 4, 8], dtype=np.uint32)


def nibbles_to_words(nib):
    """(n, 32) nibbles in base order -> (n, 4) SEQ dwords as the shard stores them"""
    by = ((nib[:, 0::2] << 4) | nib[:, 1::2]).astype(np.uint8)
    return by.view("<u4").reshape(-1, 4)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_words(packer, seed):
    """every nibble value, at every density of non-ACGT bases, and every read length within the word (0..32)"""
    rng = np.random.default_rng(seed)
    n = 20000
    acgt = ACGT[rng.integers(0, 4, size=(n, 32))]
    other = rng.integers(0, 16, size=(n, 32)).astype(np.uint32)       # 0, N (15) and the IUPAC codes among them
    frac = rng.choice([0.0, 0.01, 0.2, 1.0], size=(n, 1))
    nib = np.where(rng.random((n, 32)) < frac, other, acgt).astype(np.uint32)
    n_valid = rng.integers(0, 33, size=n).astype(np.uint32)
    words = nibbles_to_words(nib)
    got, want = packer(words, n_valid), model(words, n_valid)
    bad_rows = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad_rows) == 0, (bad_rows[:5], got[bad_rows[:5]], want[bad_rows[:5]], n_valid[bad_rows[:5]])


def test_reads_as_packed(packer):
    """whole reads of odd and even lengths around 32 / 64, packed as BAM packs them (pad nibble 0 on an odd length, the last dword
    zero-filled), cut into plane words the way mkp_call_plane cuts them: the codes decode back to the read, N only where the read has one"""
    rng = np.random.default_rng(7)
    alphabet = np.array(list("ACGTN=MRWSYKVHDB"))
    bam = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
    for L in [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 127, 129]:
        p = np.where(rng.random(L) < 0.9, rng.integers(0, 4, L), rng.integers(4, 16, L))
        seq = "".join(alphabet[p])
        nib = np.array([bam[c] for c in seq] + [0] * (-L % 32), dtype=np.uint32)   # pad nibble and dword fill
        nw = (L + 31) // 32
        words = nibbles_to_words(nib.reshape(nw, 32))
        n_valid = np.array([min(32, L - 32 * w) for w in range(nw)], dtype=np.uint32)
        got = packer(words, n_valid)
        assert (got == model(words, n_valid)).all(), L
        for k, ch in enumerate(seq):
            w, b = divmod(k, 32)
            flagged = (int(got[w, 2]) >> b) & 1
            assert flagged == (ch not in "ACGT"), (L, k, ch)
            if ch in "ACGT":
                c = (int(got[w, 0 if b < 16 else 1]) >> (2 * (b % 16))) & 3
                assert "ACGT"[c] == ch, (L, k, ch, c)
        assert (got[:, 2] >> np.minimum(n_valid, 31).astype(np.uint32) == 0)[n_valid < 32].all()   # nothing flagged past the read
        # the builder's flag bitmap of a base: eq & ~bad & the read's bases == where the read has that base
        for k, ch in enumerate("ACGT"):
            for w in range(nw):
                valid = 0xffffffff if n_valid[w] >= 32 else (1 << int(n_valid[w])) - 1
                want = sum(1 << b for b in range(32) if 32 * w + b < L and seq[32 * w + b] == ch)
                assert int(got[w, 4 + k]) & ~int(got[w, 2]) & valid == want, (L, w, ch)
