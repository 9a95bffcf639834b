"""What both packers write into the 16-bit CIGAR array and the read flags (MKP_RF_CIGW), record by record on the CPU: the device ingest's
per-thread code (ingest_parse_record / ingest_pack_record / ingest_copy_record of modkit_amd/csrc/mkp_ingest_dev.hpp, compiled for the
host, the copy run lane by lane as its wave) and the host packer (Packer::add, mkp_pack.hpp) over the same hand-built BAM records:

  records WITHOUT a CIGAR of 50 and 5 000 bases — both packers give them one soft clip over the bases; the pileup never keeps such a
  record, so no GPU test ever reads its entry: 50S fits 16 bits, 5000S does not and must set the flag;
  CIGARs of 1, 2, 3, 5, 64, 129 ops (the copy moves two ops per lane and step: odd and even counts, more pairs than lanes) with an op of
  4 095 or 4 096 bases at the first, a middle and the last index.

Checked against the format's definition: entry k == (len << 4) | op for every op that fits, the flag == "some op is longer than 4 095",
the 32-bit words verbatim, the read's offset in the array a multiple of four, nothing written outside the read's room."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#define MKP_INGEST_HOST_SHIM
#include "mkp_pack.hpp"
#include "mkp_ingest_dev.hpp"
#include <cstdio>
#include <vector>
using namespace mkp;
// stdin-free: argv[1] = file of BAM records (block_size + body each), argv[2] = output.  Per record, device then host:
//   flags, cigar16_off, n_cigar, room, then n_cigar 32-bit words, then `room` 16-bit entries (as u32), then the two guard entries around the room
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); std::vector<uint8_t> raw; { uint8_t b[4096]; size_t n; while ((n = fread(b, 1, sizeof b, f)) > 0) raw.insert(raw.end(), b, b + n); }
  fclose(f); raw.resize(raw.size() + 64);
  FILE* o = fopen(argv[2], "wb");
  MkpIngestParams P; memset(&P, 0, sizeof(P)); P.raw_len = raw.size(); P.tid = 0; P.beg = 0; P.end = 0x7fffff00; P.n_ref = 1;
  Packer pk; ShardHost S; S.tid = 0;
  uint32_t c16_at = 8;   // the device record's offset in the 16-bit array: a multiple of four, as the size scan gives
  for (unsigned long long off = 0; off + 36 < raw.size() - 64;) {
    int32_t bs; memcpy(&bs, &raw[off], 4);
    MkpIngestTotals tot; memset(&tot, 0, sizeof(tot));
    MkpRecInfo R; ingest_parse_record(raw.data(), off, P, nullptr, &R, &tot.err);
    if (tot.err || (R.kind != 1 && R.kind != 3)) { fprintf(stderr, "record at %llu: err %u kind %u\n", off, tot.err, R.kind); return 1; }
    const uint32_t n = ingest_cigar_words(R.n_cigar), room = mkp_cigar16_room(n);
    std::vector<MkpReadHdr> hdr(1); std::vector<uint32_t> cigar(n + 8, 0xdeadbeefu), chunk(2 * ingest_chunk_pairs(R.n_cigar) + 2), ranks(R.ml_n + 1);
    std::vector<uint16_t> c16(c16_at + room + 8, 0xabcd); std::vector<uint8_t> seq(ingest_seq_bytes(R.l_seq) + 4), ml(R.ml_n + 1);
    std::vector<MkpTagRef> tagref(MKP_MAX_TAGS + 1); std::vector<MkpRecDigest> dig(2);
    ingest_pack_record(raw.data(), R, 0, 0, 4, 0, 0, 0, hdr.data(), chunk.data(), tagref.data(), ranks.data(), dig.data(), &tot, c16_at);
    for (uint32_t lane = 64; lane-- > 0;) ingest_copy_record(raw.data(), R, 4, 0, 0, cigar.data(), seq.data(), ml.data(), lane, 64u, c16.data(), c16_at);
    if (tot.err) { fprintf(stderr, "pack err %u\n", tot.err); return 1; }
    auto emit = [&](uint32_t flags, uint32_t coff, const uint32_t* words, const uint16_t* ent, uint32_t before, uint32_t after) {
      const uint32_t head[4] = {flags, coff, n, room}; fwrite(head, 4, 4, o); fwrite(words, 4, n, o);
      for (uint32_t k = 0; k < room; k++) { const uint32_t e = ent[k]; fwrite(&e, 4, 1, o); }
      const uint32_t g[2] = {before, after}; fwrite(g, 4, 2, o); };
    if (cigar[3] != 0xdeadbeefu || cigar[4 + n] != 0xdeadbeefu) { fprintf(stderr, "32-bit words written outside the read\n"); return 1; }
    emit(hdr[0].flags, hdr[0].cigar16_off & ~3u, cigar.data() + 4, c16.data() + c16_at, c16[c16_at - 1], c16[c16_at + room]);
    // the host packer on the same record
    mkp_record r; memset(&r, 0, sizeof(r)); const uint8_t* c = &raw[off + 4];
    memcpy(&r.tid, c, 4); memcpy(&r.pos, c + 4, 4); r.l_qname = c[8]; uint16_t nc; memcpy(&nc, c + 12, 2); r.n_cigar = nc; memcpy(&r.flag, c + 14, 2);
    memcpy(&r.l_qseq, c + 16, 4); r.l_data = bs - 32; r.data = c + 32;
    const size_t before = S.cigar16.size();
    pk.add(r, S);
    const MkpReadHdr& h = S.hdr.back();
    if (h.cigar16_off != before || S.cigar16.size() != before + room || h.n_cigar != n) { fprintf(stderr, "host room\n"); return 1; }
    emit(h.flags, h.cigar16_off, S.cigar.data() + h.cigar_off, S.cigar16.data() + h.cigar16_off, 0xabcd, 0xabcd);
    off += 4 + (unsigned long long)bs; c16_at += 4;
  }
  fclose(o); return 0;
}
"""

RF_REVERSE, RF_CIGW = 1, 32
OPS = "MIDNSHP=X"


def bam_record(pos, flag, cigar, l_seq, name=b"r\0"):
    cg = b"".join(struct.pack("<I", (n << 4) | OPS.index(op)) for n, op in cigar)
    body = struct.pack("<iiBBHHHiiii", 0, pos, len(name), 60, 4680, len(cigar), flag, l_seq, -1, -1, 0) + name + cg + b"\x12" * ((l_seq + 1) // 2) + b"\xff" * l_seq
    return struct.pack("<i", len(body)) + body


def gapped(n_ops, special):
    """n_ops ops that start and end on a match (odd counts; even ones get a leading soft clip), `special` = {index: length} on match slots"""
    ops = [(3, "S")] if n_ops % 2 == 0 else []
    first = len(ops)
    for i in range(first, n_ops):
        ops.append((special.get(i, 2 + i % 7), "M") if (i - first) % 2 == 0 else (1 + i % 3, "DI"[i % 2]))
    return ops


def cases():
    out = [("no CIGAR, 50 bases", 0, [], 50), ("no CIGAR, 5000 bases, reverse", 16, [], 5000), ("no CIGAR, 4095 bases", 0, [], 4095),
           ("no CIGAR, 4096 bases", 0, [], 4096)]
    for n_ops in (1, 2, 3, 5, 64, 129):
        first = 1 if n_ops % 2 == 0 else 0
        slots = sorted({first, first + 2 * ((n_ops - 1 - first) // 4), n_ops - 1})
        for at in slots:
            for length in (4095, 4096):
                ops = gapped(n_ops, {at: length})
                l_seq = sum(n for n, op in ops if op in "MIS=X")
                out.append(("%d ops, %d at %d" % (n_ops, length, at), 16 if at % 2 else 0, ops, l_seq))
    return out


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    d = tmp_path_factory.mktemp("cigar16_packers")
    src, exe, inp, outp = d / "h.cpp", d / "h", d / "recs.bin", d / "out.bin"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "modkit_amd", "csrc"), "-o", str(exe), str(src), "-lz", "-lpthread"])
    cs = cases()
    inp.write_bytes(b"".join(bam_record(100 + 7 * i, flag, cigar, l_seq) for i, (_, flag, cigar, l_seq) in enumerate(cs)))
    subprocess.check_call([str(exe), str(inp), str(outp)])
    words = struct.unpack("<%dI" % (os.path.getsize(outp) // 4), outp.read_bytes())
    res, at = [], 0
    for _ in cs:
        pair = []
        for _side in range(2):
            flags, coff, n, room = words[at:at + 4]
            w = words[at + 4:at + 4 + n]
            e = words[at + 4 + n:at + 4 + n + room]
            guard = words[at + 4 + n + room:at + 6 + n + room]
            pair.append((flags, coff, n, room, w, e, guard))
            at += 6 + n + room
        res.append(pair)
    assert at == len(words)
    return cs, res


def test_both_packers_write_the_entries_and_the_flag(packed):
    cs, res = packed
    assert len(cs) >= 30
    n_wide = 0
    for (what, flag, cigar, l_seq), pair in zip(cs, res):
        ops = cigar or [(l_seq, "S")]                              # a record without a CIGAR: one soft clip over its bases
        want_words = tuple((n << 4) | OPS.index(op) for n, op in ops)
        wide = any(n > 4095 for n, _ in ops)
        n_wide += wide
        for side, (flags, coff, n, room, w, e, guard) in zip(("device", "host"), pair):
            assert n == len(ops) and room == (n + 3) // 4 * 4 and coff % 4 == 0, (what, side)
            assert w == want_words, (what, side)
            assert bool(flags & RF_CIGW) == wide, (what, side, flags)
            assert bool(flags & RF_REVERSE) == bool(flag & 16), (what, side)
            for k, (length, op) in enumerate(ops):
                if length <= 4095:                                 # (an op that does not fit leaves an entry nobody decodes)
                    assert e[k] == ((length << 4) | OPS.index(op)) and e[k] == want_words[k], (what, side, k)
            assert guard == (0xabcd, 0xabcd), (what, side, "written outside the read's room")
        assert pair[0][0] == pair[1][0], (what, "device and host flags differ")
    assert 10 < n_wide < len(cs) - 10


def test_the_records_without_a_cigar(packed):
    """the two the GPU suite cannot see: 50S is entry (50 << 4) | 4 without the flag; 5000S sets the flag on both packers"""
    cs, res = packed
    by = {what: pair for (what, _, _, _), pair in zip(cs, res)}
    for side in (0, 1):
        flags, _, n, room, w, e, _ = by["no CIGAR, 50 bases"][side]
        assert n == 1 and room == 4 and w == ((50 << 4) | 4,) and e[0] == (50 << 4) | 4 and not flags & RF_CIGW
        flags, _, n, room, w, e, _ = by["no CIGAR, 5000 bases, reverse"][side]
        assert n == 1 and room == 4 and w == ((5000 << 4) | 4,) and flags & RF_CIGW and flags & RF_REVERSE
        assert not by["no CIGAR, 4095 bases"][side][0] & RF_CIGW and by["no CIGAR, 4095 bases"][side][5][0] == (4095 << 4) | 4
        assert by["no CIGAR, 4096 bases"][side][0] & RF_CIGW
