"""The 16-bit CIGAR of the slot decoder (modkit_amd/csrc/mkp_cigar_pack.hpp: one uint16 per op, (len << 4) | op for len <= 4 095)
compiled for the host with g++ and compared with a numpy model: every op code at lengths on both sides of every field edge, the
fits / does-not-fit predicate per op and per read, and the room a read takes in the array."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "mkp_cigar_pack.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb");
  // per read: n_cigar, then its words -> per op {fits, packed, unpacked}, then per read {wide, room}
  uint32_t n;
  while (fread(&n, 4, 1, f) == 1) {
    std::vector<uint32_t> w(n);
    if (n && fread(w.data(), 4, n, f) != n) return 1;
    for (uint32_t k = 0; k < n; k++) {
      const uint16_t e = mkp_cigar16_pack(w[k]);
      const uint32_t out[3] = {mkp_cigar16_fits(w[k]) ? 1u : 0u, e, mkp_cigar16_unpack(e)};
      fwrite(out, 4, 3, o);
    }
    const uint32_t tail[3] = {mkp_cigar16_read_wide(w.data(), n) ? 1u : 0u, mkp_cigar16_room(n), MKP_CIGAR16_MAX_LEN};
    fwrite(tail, 4, 3, o);
  }
  fclose(f); fclose(o); return 0;
}
"""

OPS = range(9)                                     # M I D N S H P = X
LENGTHS = [1, 15, 16, 127, 128, 4095, 4096, 65535, 65536, (1 << 28) - 1]


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    d = tmp_path_factory.mktemp("cigar_pack")
    src, exe = d / "pack.cpp", d / "pack"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "modkit_amd", "csrc"), "-o", str(exe), str(src)])

    def run(reads):
        """reads: lists of BAM CIGAR words -> (per read: (n, 3) array of {fits, packed, unpacked}, (wide, room, max_len))"""
        inp, out = d / "in.bin", d / "out.bin"
        with open(inp, "wb") as f:
            for words in reads:
                np.array([len(words)] + list(words), dtype="<u4").tofile(f)
        subprocess.check_call([str(exe), str(inp), str(out)])
        flat, res, at = np.fromfile(out, dtype="<u4").reshape(-1, 3), [], 0
        for words in reads:
            res.append((flat[at:at + len(words)], tuple(int(x) for x in flat[at + len(words)])))
            at += len(words) + 1
        assert at == len(flat)
        return res
    return run


def model_op(length, op):
    """(fits, the 16-bit entry) of one op, from the format's definition"""
    fits = length <= 4095
    return fits, ((length << 4) | op) if fits else None


def test_every_op_code_at_every_length(packer):
    reads = [[(n << 4) | op] for op in OPS for n in LENGTHS]
    got = packer(reads)
    k = 0
    for op in OPS:
        for n in LENGTHS:
            (per_op, (wide, room, max_len)), k = got[k], k + 1
            fits, entry = model_op(n, op)
            assert max_len == 4095
            assert bool(per_op[0, 0]) == fits, (op, n)
            assert bool(wide) == (not fits), (op, n)                # a read of this one op
            assert room == 4
            if fits:
                assert int(per_op[0, 1]) == entry and entry < (1 << 16), (op, n)
                assert int(per_op[0, 2]) == ((n << 4) | op), (op, n)   # widened back: the BAM word
                assert int(per_op[0, 2]) >> 4 == n and int(per_op[0, 2]) & 15 == op


def test_predicate_either_side_of_the_limit(packer):
    """4 095 fits, 4 096 does not; one op over the limit anywhere in a read makes the read wide, and no other read"""
    short = [(n << 4) | (k % 3) for k, n in enumerate([1, 4095, 17, 300, 4095, 2, 4095])]
    reads = [short]
    for at in (0, 3, len(short) - 1):
        for n in (4095, 4096):
            w = list(short)
            w[at] = (n << 4) | (w[at] & 15)
            reads.append(w)
    reads.append([])                                             # (no ops: nothing to be wide)
    got = packer(reads)
    assert got[0][1][0] == 0 and got[0][0][:, 0].all()
    k = 1
    for at in (0, 3, len(short) - 1):
        for n in (4095, 4096):
            per_op, (wide, room, _) = got[k]; k += 1
            assert wide == (1 if n == 4096 else 0), (at, n)
            want_fits = np.ones(len(short), dtype=bool)
            want_fits[at] = n <= 4095
            assert (per_op[:, 0].astype(bool) == want_fits).all(), (at, n)
            assert room == 8
    assert got[k][1][0] == 0 and got[k][1][1] == 0


@pytest.mark.parametrize("seed", [0, 1])
def test_random_reads_round_trip(packer, seed):
    """random op codes and lengths up to 4 095: the entry is the word's low half, widening gives the word back; the room is the op count
    rounded up to four entries (every read starts on an 8-byte boundary of the array)"""
    rng = np.random.default_rng(seed)
    reads = []
    for n in [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1025]:
        lens = np.where(rng.random(n) < 0.8, rng.integers(1, 40, n), rng.integers(1, 4096, n))
        reads.append(list(((lens << 4) | rng.integers(0, 9, n)).astype(np.uint32)))
    for words, (per_op, (wide, room, _)) in zip(reads, packer(reads)):
        w = np.array(words, dtype=np.uint32)
        assert not wide and per_op[:, 0].all()
        assert (per_op[:, 1] == w).all() and (per_op[:, 1] < (1 << 16)).all() and (per_op[:, 2] == w).all()
        assert room == (len(words) + 3) // 4 * 4 and room % 4 == 0 and 0 <= room - len(words) < 4
