// Host half of `modkit dmr pair` without -r over replicates (mkp_dmr_reps.hip): the table of SingleSiteDmrScore::header(multiple, matched) /
// to_row (src/dmr/single_site.rs:436-660) on top of the 16 columns of mkp_dmr_sites.hpp.  No device: tests/dmr_reps_math_host.cpp compiles it.
#pragma once
#include <string>

#include "mkp_dmr_reps_math.hpp"
#include "mkp_dmr_sites.hpp"
#include "mkpileup.h"

namespace mkp {

inline bool dmr_reps_multiple(const mkp_dmr_reps_out& t) { return t.n_a > 1 || t.n_b > 1; }
inline bool dmr_reps_matched(const mkp_dmr_reps_out& t) { return t.n_a == t.n_b && t.n_a > 1; }

inline std::string dmr_reps_header(bool multiple, bool matched) {
  std::string s = dmr_sites_header();
  s.pop_back();
  if (multiple) s += "\tbalanced_map_pvalue\tbalanced_effect_size\tpct_a_samples\tpct_b_samples";
  if (matched) s += "\treplicate_map_pvalues\treplicate_effect_sizes";
  return s + "\n";
}

// the rows of sites [from, to): the 16 columns, with more than one sample a side the balanced values and the shares of samples, with matched
// sides the per-replicate values, comma-joined, or `-` where the site has none
template <class F32Text> void dmr_reps_rows_text(std::string& s, const mkp_dmr_reps_out& t, const char* const* contig_names, uint64_t from, uint64_t to,
    F32Text f32_text) {
  const bool multiple = dmr_reps_multiple(t), matched = dmr_reps_matched(t);
  for (uint64_t i = from; i < to; i++) {
    dmr_sites_row_text(s, t.sites, contig_names, i, f32_text);
    if (multiple) {
      s += '\t'; s += f64_display(t.balanced_map_pvalue[i]); s += '\t'; s += f64_display(t.balanced_effect_size[i]);
      for (int side = 0; side < 2; side++) { s += '\t'; s += std::to_string(t.pct_samples[side][i]); }
    }
    if (matched) for (const double* v : {t.rep_pvalue, t.rep_effect}) {
      s += '\t';
      if (!t.n_rep[i]) { s += '-'; continue; }
      for (uint32_t r = 0; r < t.n_rep[i]; r++) { if (r) s += ','; s += f64_display(v[i * t.n_a + r]); }
    }
    s += '\n';
  }
}

}  // namespace mkp
