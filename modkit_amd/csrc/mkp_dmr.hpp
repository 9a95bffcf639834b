// Host half of `modkit dmr pair` over regions: the score (llk_ratio, src/dmr/llr_model.rs:227-330), which regions are written, and the
// table (ModificationCounts::header / to_row, llr_model.rs:152-225).  No device and no other header of the library but the public one and
// the row formatter: tests/dmr_score_host.cpp compiles it alone.
#pragma once
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "mkp_format.hpp"
#include "mkpileup.h"

namespace mkp {

// MOD_CODE_TO_DNA_BASE (src/mod_base_code.rs:69-90): code_repr (a ChEBI number carries bit 31) and the index of its base in "ACGT"
struct DmrLookupEntry { uint32_t code; uint8_t base; };
inline const std::vector<DmrLookupEntry>& dmr_default_lookup() {
  constexpr uint32_t E = 0x80000000u;
  static const std::vector<DmrLookupEntry> t = {{'m', 1}, {'h', 1}, {'f', 1}, {'c', 1}, {21839u | E, 1}, {'C', 1}, {'a', 0}, {'A', 0}, {17596u | E, 0},
      {'g', 3}, {'e', 3}, {'b', 3}, {17802u | E, 3}, {'T', 3}, {'o', 2}, {'G', 2}, {16450u | E, 3}};
  return t;
}

// ln of the marginal likelihood of counts n[0 .. k) under the POSTERIOR of a Jeffreys prior updated with the same counts — what
// `prior.posterior(&data).ln_m(&data)` computes, not the marginal under the prior: the posterior is Dirichlet(1/2 + n_i) and its ln_m over
// the same data is [sum lnG(1/2 + 2 n_i) - lnG(k/2 + 2N)] - [sum lnG(1/2 + n_i) - lnG(k/2 + N)].  For k = 2 this is rv's Beta form as well.
inline double dmr_llk(const std::vector<uint64_t>& n) {
  const double k2 = 0.5 * (double)n.size();
  double N = 0, twice = 0, once = 0;
  for (uint64_t v : n) { const double x = (double)v; N += x; twice += std::lgamma(0.5 + 2.0 * x); once += std::lgamma(0.5 + x); }
  return (twice - std::lgamma(k2 + 2.0 * N)) - (once - std::lgamma(k2 + N));
}

// llk_ratio over the session's code columns: has[k] = the sample's key set holds code k (a code counted with N_mod == 0 too), mod[k] its
// count.  false: the reference fails here and drops the region (Beta branch over two different codes; counts beyond the total).
inline bool dmr_llk_ratio(const uint64_t* a_mod, const uint8_t* a_has, uint64_t a_total, const uint64_t* b_mod, const uint8_t* b_has, uint64_t b_total,
    uint32_t n_codes, double* score) {
  uint32_t ka = 0, kb = 0, ku = 0; uint64_t sa = 0, sb = 0;
  for (uint32_t k = 0; k < n_codes; k++) { if (a_has[k]) { ka++; sa += a_mod[k]; } if (b_has[k]) { kb++; sb += b_mod[k]; } if (a_has[k] || b_has[k]) ku++; }
  *score = 0.0;
  if (sa > a_total || sb > b_total) return false;   // AggregatedCounts::try_new
  const uint32_t n_categories = (ka > kb ? ka : kb) + 1u;
  if (n_categories < 2u) return true;
  if (n_categories == 2u && ku != 1u) return false;   // llk_beta: "should have exactly one modification"
  // category 0 = canonical, then the sorted union of both key sets (llk_dirichlet; llk_beta is the same with one code)
  std::vector<uint64_t> a{a_total - sa}, b{b_total - sb}, ab{a_total - sa + (b_total - sb)};
  for (uint32_t k = 0; k < n_codes; k++) if (a_has[k] || b_has[k]) { const uint64_t x = a_has[k] ? a_mod[k] : 0, y = b_has[k] ? b_mod[k] : 0;
    a.push_back(x); b.push_back(y); ab.push_back(x + y); }
  *score = dmr_llk(a) + dmr_llk(b) - dmr_llk(ab);
  return true;
}

// which regions are written and their scores: fills score[r] and state[r] (MKP_DMR_* of mkpileup.h) from the other fields of `t`
inline void dmr_judge(const mkp_dmr_out& t, double* score, uint8_t* state) {
  for (uint32_t r = 0; r < t.n_regions; r++) {
    score[r] = 0.0;
    const size_t at = (size_t)r * t.n_codes;
    if (!t.contig_has_rows[0][r] || !t.contig_has_rows[1][r]) state[r] = MKP_DMR_NO_CONTIG;
    else if (!t.has_reference[r]) state[r] = MKP_DMR_NO_REFERENCE;
    else if (t.bad[0][r] || t.bad[1][r]) state[r] = MKP_DMR_BAD;
    else state[r] = dmr_llk_ratio(t.n_mod[0] + at, t.has_code[0] + at, t.total[0][r], t.n_mod[1] + at, t.has_code[1] + at, t.total[1][r], t.n_codes,
        &score[r]) ? MKP_DMR_WRITTEN : MKP_DMR_MODEL;
  }
}

// f64 through Rust's Display: the shortest digits that parse back to the same f64, positional notation, never an exponent
inline std::string f64_display(double v) {
  if (v != v) return "NaN";
  if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
  // the shortest digits and their exponent (to_chars in fixed notation writes the exact integer of a value beyond 2^53, not the shortest
  // digits padded with zeros, which is what Rust prints), laid out positionally
  char buf[64];
  const std::to_chars_result r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::scientific);
  const std::string s(buf, r.ptr);
  const size_t e = s.find('e');
  const int ex = std::atoi(s.c_str() + e + 1);
  std::string digits; bool neg = false;
  for (size_t k = 0; k < e; k++) { if (s[k] == '-') neg = true; else if (s[k] != '.') digits.push_back(s[k]); }
  std::string out;
  if (ex >= 0) {
    if ((int)digits.size() <= ex + 1) out = digits + std::string((size_t)(ex + 1 - (int)digits.size()), '0');
    else out = digits.substr(0, (size_t)ex + 1) + "." + digits.substr((size_t)ex + 1);
  } else out = "0." + std::string((size_t)(-ex - 1), '0') + digits;
  return neg ? "-" + out : out;
}

inline std::string dmr_code_text(uint32_t code) { return (code & 0x80000000u) ? std::to_string(code & 0x7fffffffu) : std::string(1, (char)code); }

// AggregatedCounts::string_counts / string_percentages of one sample's cells of a region
inline std::string dmr_counts_text(const mkp_dmr_out& t, int sample, uint32_t r, bool percentages) {
  std::string s; const size_t at = (size_t)r * t.n_codes;
  for (uint32_t k = 0; k < t.n_codes; k++) if (t.has_code[sample][at + k]) {
    if (!s.empty()) s += ',';
    s += dmr_code_text(t.code_repr[k]); s += ':';
    if (!percentages) { s += std::to_string(t.n_mod[sample][at + k]); continue; }
    const float frac = (float)t.n_mod[sample][at + k] / (float)t.total[sample][r];
    char buf[64]; s.append(buf, put_pct2(buf, frac * 100.0f));
  }
  return s.empty() ? "." : s;
}

// The table; Set = mkp_region_set (regions, chrom, name with "." for a line without one); `f32_text` = f32 Display of a number
template <class Set, class F32Text> std::string dmr_table_text(const Set& set, const mkp_dmr_out& t, bool header, F32Text f32_text) {
  std::string s;
  if (header) s = "chrom\tstart\tend\tname\tscore\tstrand\ta_counts\ta_total\tb_counts\tb_total\ta_mod_percentages\tb_mod_percentages\ta_pct_modified\t"
      "b_pct_modified\n";
  for (uint32_t r = 0; r < t.n_regions; r++) {
    if (t.state[r] != MKP_DMR_WRITTEN) continue;
    const auto& g = set.regions[r];
    const std::string span = std::to_string(g.start) + "\t" + std::to_string(g.end);
    s += set.chrom[r]; s += '\t'; s += span; s += '\t';
    if (set.name[r] == ".") { s += set.chrom[r]; s += ':'; s += std::to_string(g.start); s += '-'; s += std::to_string(g.end); } else s += set.name[r];
    s += '\t'; s += f64_display(t.score[r]); s += '\t'; s += g.strand_rule == 1 ? '+' : g.strand_rule == 2 ? '-' : '.';
    for (int sample = 0; sample < 2; sample++) { s += '\t'; s += dmr_counts_text(t, sample, r, false); s += '\t'; s += std::to_string(t.total[sample][r]); }
    for (int sample = 0; sample < 2; sample++) { s += '\t'; s += dmr_counts_text(t, sample, r, true); }
    for (int sample = 0; sample < 2; sample++) {   // pct_modified: modified / total as f32, a fraction; 0 / 0 prints NaN
      uint64_t m = 0; for (uint32_t k = 0; k < t.n_codes; k++) if (t.has_code[sample][(size_t)r * t.n_codes + k]) m += t.n_mod[sample][(size_t)r * t.n_codes + k];
      const float f = (float)m / (float)t.total[sample][r];
      s += '\t'; s += f != f ? std::string("NaN") : std::isinf(f) ? std::string("inf") : f32_text(f);
    }
    s += '\n';
  }
  return s;
}

}  // namespace mkp
