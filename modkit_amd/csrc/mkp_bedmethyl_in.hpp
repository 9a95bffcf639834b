// bedMethyl input for `bedmethyl merge` (BedMethylLine, src/dmr/bedmethyl.rs:40-86), host side: every count column of every line, split
// into runs of lines on one contig.  No device here; reached through the ABI as mkp_host_read_bedmethyl so that it is tested on the CPU.
// The device reader (mkp_bedmethyl.hip, driven by mkp_api.cpp) shares three things with it: the grammar of a line
// (mkp_bedmethyl_line.hpp), the walk over a BGZF file's block table (bgzf_walk) and the messages of a bad line (bedmethyl_line_error) —
// when the device finds a bad line, the host reader is run over that piece of text and throws.
//
// What is read of a line: mkp_bedmethyl_line.hpp.  Lines that start with '#' are skipped, as tabix skips them.  The file is plain text or
// bgzip (BGZF) compressed, as `modkit bedmethyl merge` takes it; its .tbi is neither needed nor read.  Here a BGZF file is inflated by the
// host's own decoder (mkp_inflate_host.hpp), every block's CRC-32 checked.  Deviations from the reference: a line that does
// not parse fails the whole file with MKP_E_IO, naming the line (the reference drops the 100 kb chunk the line lies in, silently); a gzip
// stream without BGZF blocks is MKP_E_UNSUPPORTED; a start or a count beyond 2^32 - 1 is MKP_E_UNSUPPORTED (rows carry 32-bit columns).
#pragma once
#include <fstream>
#include <string>
#include <vector>

#include "mkp_bedmethyl_line.hpp"
#include "mkp_crc32.hpp"
#include "mkp_inflate_host.hpp"
#include "mkp_pack.hpp"

struct mkp_bedmethyl_file {
  struct Run { std::string chrom; uint64_t first = 0, n = 0; };
  std::vector<Run> runs;                    // file order; a contig may come back in a later run
  // pos, code_repr, n_valid, n_mod, n_canonical, n_other, n_delete, n_fail, n_diff, n_nocall
  std::vector<uint32_t> col[10];
  std::vector<uint8_t> strand; std::vector<int32_t> motif;   // motif_idx = -1 throughout
  uint64_t n_rows() const { return col[0].size(); }
  mkp_rows rows_of(size_t run) const {
    mkp_rows r; memset(&r, 0, sizeof(r));
    const Run& u = runs[run]; const size_t f = (size_t)u.first;
    r.n_rows = u.n; r.pos = col[0].data() + f; r.strand = strand.data() + f; r.code_repr = col[1].data() + f; r.motif_idx = motif.data() + f;
    r.n_valid = col[2].data() + f; r.n_mod = col[3].data() + f; r.n_canonical = col[4].data() + f; r.n_other = col[5].data() + f;
    r.n_delete = col[6].data() + f; r.n_fail = col[7].data() + f; r.n_diff = col[8].data() + f; r.n_nocall = col[9].data() + f;
    return r;
  }
};

namespace mkp {

inline bool is_gzip(const uint8_t* z, size_t n) { return n >= 2 && z[0] == 0x1f && z[1] == 0x8b; }

// one block of a BGZF file: the deflate payload [in_off, in_off + in_len), its CRC-32 and ISIZE, and the block's own extent
struct BgzfBlk { uint64_t start; uint32_t bsize; uint64_t in_off; uint32_t in_len, crc, isize; };

// The block table of a BGZF file held in memory (SAM spec §4.1: gzip members whose FEXTRA holds a `BC` subfield with the block size).
// A gzip stream whose first member has no such subfield is not BGZF: MKP_E_UNSUPPORTED.  A truncated block or a bad header further on is
// MKP_E_IO naming the block.  Blocks with ISIZE 0 are listed like the others (the EOF block is one; bgzip may write them anywhere).
inline std::vector<BgzfBlk> bgzf_walk(const uint8_t* z, size_t n, const std::string& path) {
  std::vector<BgzfBlk> blks;
  for (uint64_t o = 0; o < n;) {
    const std::string where = "BGZF block " + std::to_string(blks.size()) + " of " + path;
    auto not_bgzf = [&]() { return blks.empty() ? Error(MKP_E_UNSUPPORTED, path + " is gzip compressed without BGZF blocks: bedmethyl merge reads"
        " plain text or bgzip output") : Error(MKP_E_IO, "bad header of " + where); };
    if (o + 18 > n) { if (blks.empty() && n >= 4 && (z[2] != 8 || !(z[3] & 4))) throw not_bgzf(); throw Error(MKP_E_IO, "truncated " + where); }
    if (z[o] != 31 || z[o + 1] != 139 || z[o + 2] != 8 || !(z[o + 3] & 4)) throw not_bgzf();
    uint16_t xlen; memcpy(&xlen, z + o + 10, 2);
    uint64_t x = o + 12; const uint64_t xe = x + xlen; uint32_t bsize = 0; bool found = false;
    if (xe > n) throw Error(MKP_E_IO, "truncated " + where);
    while (x + 4 <= xe) { uint16_t sl; memcpy(&sl, z + x + 2, 2);
      if (z[x] == 'B' && z[x + 1] == 'C' && sl == 2 && x + 6 <= xe) { uint16_t b; memcpy(&b, z + x + 4, 2); bsize = (uint32_t)b + 1; found = true; }
      x += 4 + (uint64_t)sl; }
    if (!found) throw not_bgzf();
    if (bsize < (uint32_t)xlen + 20u) throw Error(MKP_E_IO, "bad header of " + where);
    if (o + bsize > n) throw Error(MKP_E_IO, "truncated " + where);
    BgzfBlk b; b.start = o; b.bsize = bsize; b.in_off = o + 12 + xlen; b.in_len = bsize - xlen - 20;
    memcpy(&b.crc, z + o + bsize - 8, 4); memcpy(&b.isize, z + o + bsize - 4, 4);
    if (b.isize > 65536u) throw Error(MKP_E_IO, where + " inflates to more than 64 KiB");
    blks.push_back(b); o += bsize;
  }
  return blks;
}

// block k of the table inflated into dst[0, isize) by the host decoder, its CRC-32 checked
inline void bgzf_inflate_block_host(const uint8_t* z, const BgzfBlk& b, size_t k, uint8_t* dst, const std::string& path) {
  uint8_t none = 0;
  if (!hostinf::inflate(z + b.in_off, b.in_len, b.isize ? dst : &none, b.isize)) throw Error(MKP_E_IO,
      "corrupt BGZF data: block " + std::to_string(k) + " of " + path + " does not inflate");
  if (crc32_of(b.isize ? dst : &none, b.isize) != b.crc) throw Error(MKP_E_IO,
      "corrupt BGZF data: block " + std::to_string(k) + " of " + path + " (CRC-32 mismatch)");
}

// what a finding of mkp_bedmethyl_parse_line is called, and its status
inline Error bedmethyl_line_error(uint32_t code, uint64_t line_no, const std::string& path, const uint8_t* line, size_t len) {
  if (len && line[len - 1] == '\r') len--;
  const std::string field = std::to_string(MKP_BML_FIELD(code));
  int st = MKP_E_IO; std::string why;
  switch (MKP_BML_CLASS(code)) {
    case MKP_BML_FEW_FIELDS: why = "failed to parse bedMethyl line (fewer than 18 fields)"; break;
    case MKP_BML_NOT_NUMBER: why = "failed to parse bedMethyl line (field " + field + " is not a number)"; break;
    case MKP_BML_BEYOND_32: st = MKP_E_UNSUPPORTED; why = "field " + field + " is beyond 2^32 - 1"; break;
    case MKP_BML_BAD_CODE: why = "failed to parse bedMethyl line (invalid mod code representation)"; break;
    case MKP_BML_BAD_STRAND: why = "failed to parse bedMethyl line (strand must be +, - or .)"; break;
    default: why = "failed to parse bedMethyl line"; break;
  }
  return Error(st, "line " + std::to_string(line_no) + " of " + path + ": " + why + ": " + std::string((const char*)line, std::min<size_t>(len, 200)));
}

// The lines of text[0, n) appended to `out`; the first line is line `line_base` + 1 of the file (messages).  A run goes on from the last
// one of `out` when the chrom is the same.  line_nos (may be NULL): the line number of every row appended.  Returns the physical lines.
inline uint64_t parse_bedmethyl_text(const uint8_t* text, size_t n, const std::string& path, uint64_t line_base, mkp_bedmethyl_file& out,
    std::vector<uint64_t>* line_nos = nullptr) {
  uint64_t line_no = line_base;
  for (size_t p = 0; p < n;) {
    const uint8_t* nl = (const uint8_t*)memchr(text + p, '\n', n - p);
    const size_t e = nl ? (size_t)(nl - text) : n;
    line_no++;
    const size_t l0 = p; p = e + 1;
    if (e > l0 && text[l0] == '#') continue;
    if (e - l0 > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "line " + std::to_string(line_no) + " of " + path + " is longer than 2^32 - 1 bytes");
    MkpBedLine L;
    const uint32_t code = mkp_bedmethyl_parse_line(text + l0, (uint32_t)(e - l0), &L);
    if (code) throw bedmethyl_line_error(code, line_no, path, text + l0, e - l0);
    if (out.runs.empty() || out.runs.back().chrom.size() != L.chrom_len || memcmp(out.runs.back().chrom.data(), text + l0 + L.chrom_off, L.chrom_len)) {
      mkp_bedmethyl_file::Run r; r.chrom.assign((const char*)text + l0 + L.chrom_off, L.chrom_len); r.first = out.n_rows(); out.runs.push_back(r); }
    out.runs.back().n++;
    const uint32_t v[10] = {L.pos, L.code, L.n_valid, L.n_mod, L.n_canonical, L.n_other, L.n_delete, L.n_fail, L.n_diff, L.n_nocall};
    for (int k = 0; k < 10; k++) out.col[k].push_back(v[k]);
    out.strand.push_back((uint8_t)"+-."[L.strand]); out.motif.push_back(-1);
    if (line_nos) line_nos->push_back(line_no);
  }
  return line_no - line_base;
}

inline std::vector<uint8_t> read_whole_file(const std::string& path, const char* what) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(MKP_E_IO, std::string("failed to open ") + what + " " + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

inline mkp_bedmethyl_file read_bedmethyl_text(const std::string& path) {
  std::vector<uint8_t> data = read_whole_file(path, "bedMethyl");
  if (is_gzip(data.data(), data.size())) {
    const std::vector<BgzfBlk> blks = bgzf_walk(data.data(), data.size(), path);
    std::vector<uint64_t> off(blks.size() + 1, 0);
    for (size_t k = 0; k < blks.size(); k++) off[k + 1] = off[k] + blks[k].isize;
    std::vector<uint8_t> text(off.back());
    HostPool::get().parallel(blks.size(), [&](size_t k) { bgzf_inflate_block_host(data.data(), blks[k], k, text.data() + off[k], path); });
    data.swap(text);
  }
  mkp_bedmethyl_file out;
  parse_bedmethyl_text(data.data(), data.size(), path, 0, out);
  return out;
}

}  // namespace mkp
