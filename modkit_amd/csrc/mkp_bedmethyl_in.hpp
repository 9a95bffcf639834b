// Plain-text bedMethyl input for `bedmethyl merge` (BedMethylLine, src/dmr/bedmethyl.rs:40-86): every count column of every line, split
// into runs of lines on one contig.  No device here; reached through the ABI as mkp_host_read_bedmethyl so that it is tested on the CPU.
//
// What is read of a line: 18 or more fields separated by runs of tabs and / or blanks (the default and the --mixed-delim form); field 1
// chrom, 2 start, 4 name — the mod code is the name up to its first comma (consume_string_from_list, src/parsing_utils.rs:30-35), so the
// motif part of an `m,CG,0` name is not kept —, 5 score = valid_coverage (the reference takes it from the score, not from field 10),
// 6 strand, 12-18 the seven other counts.  Lines that start with '#' are skipped, as tabix skips them.  Deviations from the reference
// (DESIGN §6): a line that does not parse fails the whole file with MKP_E_IO, naming the line (the reference drops the 100 kb chunk the
// line lies in, silently); a file that starts with the gzip magic is MKP_E_UNSUPPORTED (bgzip input is not read); a start or a count beyond
// 2^32 - 1 is MKP_E_UNSUPPORTED (rows carry 32-bit columns).
#pragma once
#include <fstream>
#include <string>
#include <vector>

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

inline mkp_bedmethyl_file read_bedmethyl_text(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(MKP_E_IO, "failed to open bedMethyl " + path);
  std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (text.size() >= 2 && (uint8_t)text[0] == 0x1f && (uint8_t)text[1] == 0x8b) throw Error(MKP_E_UNSUPPORTED,
      path + " is gzip / bgzip compressed: bedmethyl merge reads plain text");
  mkp_bedmethyl_file out;
  auto sep = [](char c) { return c == ' ' || c == '\t'; };
  size_t line_no = 0;
  for (size_t p = 0; p < text.size();) {
    size_t e = text.find('\n', p); if (e == std::string::npos) e = text.size();
    size_t le = e; if (le > p && text[le - 1] == '\r') le--;
    line_no++;
    const size_t l0 = p; p = e + 1;
    if (le > l0 && text[l0] == '#') continue;
    auto bad = [&](int st, const std::string& why) { return Error(st, "line " + std::to_string(line_no) + " of " + path + ": " + why + ": "
        + text.substr(l0, std::min<size_t>(le - l0, 200))); };
    // the first 18 fields
    size_t fs[18], fe[18]; int nf = 0;
    for (size_t i = l0; i < le && nf < 18;) {
      while (i < le && sep(text[i])) i++;
      if (i >= le) break;
      fs[nf] = i; while (i < le && !sep(text[i])) i++; fe[nf++] = i;
    }
    if (nf < 18) throw bad(MKP_E_IO, "failed to parse bedMethyl line (fewer than 18 fields)");
    auto number = [&](int k) -> uint32_t {
      uint64_t v = 0; if (fe[k] == fs[k]) throw bad(MKP_E_IO, "failed to parse bedMethyl line");
      for (size_t i = fs[k]; i < fe[k]; i++) { const char c = text[i];
        if (c < '0' || c > '9') throw bad(MKP_E_IO, "failed to parse bedMethyl line (field " + std::to_string(k + 1) + " is not a number)");
        v = v * 10 + (uint64_t)(c - '0');
        if (v > 0xffffffffull) throw bad(MKP_E_UNSUPPORTED, "field " + std::to_string(k + 1) + " is beyond 2^32 - 1"); }
      return (uint32_t)v;
    };
    const uint32_t start = number(1); (void)number(2);
    // ModCodeRepr::parse (src/mod_base_code.rs:112-122) of the name up to its first comma: one character, or a ChEBI number
    size_t ce = fs[3]; while (ce < fe[3] && text[ce] != ',') ce++;
    uint32_t code = 0;
    if (ce - fs[3] == 1) code = (uint32_t)(unsigned char)text[fs[3]];
    else { uint64_t v = 0; bool ok = ce > fs[3];
      for (size_t i = fs[3]; i < ce && ok; i++) { ok = text[i] >= '0' && text[i] <= '9'; v = v * 10 + (uint64_t)(text[i] - '0'); ok = ok && v <= 0x7fffffffull; }
      if (!ok) throw bad(MKP_E_IO, "failed to parse bedMethyl line (invalid mod code representation)");
      code = 0x80000000u | (uint32_t)v; }
    if (!code) throw bad(MKP_E_IO, "failed to parse bedMethyl line (invalid mod code representation)");
    const uint32_t n_valid = number(4);
    if (fe[5] - fs[5] != 1 || (text[fs[5]] != '+' && text[fs[5]] != '-' && text[fs[5]] != '.')) throw bad(MKP_E_IO,
        "failed to parse bedMethyl line (strand must be +, - or .)");
    (void)number(6); (void)number(7); (void)number(9);
    const std::string chrom = text.substr(fs[0], fe[0] - fs[0]);
    if (out.runs.empty() || out.runs.back().chrom != chrom) { mkp_bedmethyl_file::Run r; r.chrom = chrom; r.first = out.n_rows(); out.runs.push_back(r); }
    out.runs.back().n++;
    out.col[0].push_back(start); out.col[1].push_back(code); out.col[2].push_back(n_valid);
    for (int k = 0; k < 7; k++) out.col[3 + k].push_back(number(11 + k));
    out.strand.push_back((uint8_t)text[fs[5]]); out.motif.push_back(-1);
  }
  return out;
}

}  // namespace mkp
