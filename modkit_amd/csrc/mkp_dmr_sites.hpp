// Host half of `modkit dmr pair` without -r (mkp_dmr_sites.hip): the batch planner (SingleSiteBatches::get_next_batch,
// src/dmr/single_site.rs:349-407), one site's values through the shared arithmetic, and the table (SingleSiteDmrScore::to_row_pair,
// single_site.rs:608-659).  No device and no other header of the library but the public one, the maths and the formatters:
// tests/dmr_site_math_host.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mkp_dmr.hpp"
#include "mkp_dmr_site_math.hpp"
#include "mkpileup.h"

namespace mkp {

inline uint64_t dmr_sites_windows(uint64_t contig_len, uint64_t interval) { return std::max<uint64_t>(1, (contig_len + interval - 1) / interval); }

// The reference's walk over the contigs (already in its order): every contig in windows of `interval` bp, a batch collecting windows until it
// holds `interval` listed positions, running on into the next contig; what is unfinished at the very end is a batch.  (A super-batch ends
// right behind a finished batch, so super-batches do not move a boundary.)  counts: the listed positions per window, one contig behind the
// other.  An entry = where a batch begins inside a contig.  Returns the number of batches.
inline uint64_t dmr_sites_plan(const uint64_t* contig_len, const uint32_t* counts, uint32_t n_contigs, uint64_t interval,
    std::vector<mkp_dmr_sites_batch>* entries) {
  uint64_t batch = 0, held = 0, w = 0; bool open = false;   // open: the current batch holds a window
  for (uint32_t c = 0; c < n_contigs; c++) {
    const uint64_t nw = dmr_sites_windows(contig_len[c], interval);
    bool listed_here = false;   // the current batch has its entry for this contig
    for (uint64_t k = 0; k < nw; k++, w++) {
      if (!listed_here) { entries->push_back({c, 0u, k * interval, batch}); listed_here = true; }
      held += counts[w]; open = true;
      if (held >= interval) { batch++; held = 0; open = false; listed_here = false; }
    }
  }
  return batch + (open ? 1u : 0u);
}

// one site on the host: values = score, ln_effect, ln_null, map_pvalue, effect_size; false = the reference fails on it
inline bool dmr_site_score(const uint64_t* a_mod, uint32_t a_has, uint64_t a_total, const uint64_t* b_mod, uint32_t b_has, uint64_t b_total,
    uint32_t n_codes, const MkpDmrSiteMath& M, double* values) {
  uint64_t ma = 0, mb = 0;
  for (uint32_t k = 0; k < n_codes; k++) { if ((a_has >> k) & 1u) ma += a_mod[k]; if ((b_has >> k) & 1u) mb += b_mod[k]; }
  bool ok = dmr_site_pmap(M, ma, a_total, mb, b_total, &values[1], &values[2], &values[3], &values[4]);
  ok = dmr_site_llk_ratio<uint64_t>(a_mod, a_has, a_total, b_mod, b_has, b_total, n_codes, &values[0]) && ok;
  return ok;
}

inline MkpDmrSiteMath dmr_site_math(double alpha, double beta, double delta, const uint32_t max_cov[2]) {
  MkpDmrSiteMath M; M.alpha = alpha; M.beta = beta; M.delta = delta;
  for (int s = 0; s < 2; s++) M.max_cov[s] = std::min<uint32_t>(max_cov[s], MKP_DMR_SITE_MAX_COV);
  dmr_gauss_legendre(M.gl_x, M.gl_w);
  return M;
}

inline const char* dmr_sites_header() {
  return "chrom\tstart\tend\tname\tscore\tstrand\ta_counts\ta_total\tb_counts\tb_total\ta_mod_percentages\tb_mod_percentages\ta_pct_modified\t"
      "b_pct_modified\tmap_pvalue\teffect_size\n";
}

// AggregatedCounts::string_counts / string_percentages of one sample of a site
inline void dmr_sites_counts_text(std::string& s, const mkp_dmr_sites_out& t, int sample, uint64_t i, bool percentages) {
  bool any = false;
  for (uint32_t k = 0; k < t.n_codes; k++) if ((t.has_code[sample][i] >> k) & 1u) {
    if (any) s += ',';
    any = true;
    const uint32_t n = t.n_mod[sample][i * t.n_codes + k];
    s += dmr_code_text(t.code_repr[k]); s += ':';
    if (!percentages) { s += std::to_string(n); continue; }
    const float frac = (float)n / (float)t.total[sample][i];
    char buf[64]; s.append(buf, put_pct2(buf, frac * 100.0f));
  }
  if (!any) s += '.';
}

// the 16 fields of site i, without the line end
template <class F32Text> void dmr_sites_row_text(std::string& s, const mkp_dmr_sites_out& t, const char* const* contig_names, uint64_t i, F32Text f32_text) {
  s += contig_names[t.tid[i]]; s += '\t'; s += std::to_string(t.pos[i]); s += '\t'; s += std::to_string((uint64_t)t.pos[i] + 1); s += "\t.\t";
  s += f64_display(t.score[i]); s += '\t'; s += (char)t.strand[i];
  for (int sample = 0; sample < 2; sample++) { s += '\t'; dmr_sites_counts_text(s, t, sample, i, false); s += '\t'; s += std::to_string(t.total[sample][i]); }
  for (int sample = 0; sample < 2; sample++) { s += '\t'; dmr_sites_counts_text(s, t, sample, i, true); }
  for (int sample = 0; sample < 2; sample++) {   // pct_modified: modified / total as f32, a fraction; 0 / 0 prints NaN
    uint64_t m = 0; for (uint32_t k = 0; k < t.n_codes; k++) if ((t.has_code[sample][i] >> k) & 1u) m += t.n_mod[sample][i * t.n_codes + k];
    const float f = (float)m / (float)t.total[sample][i];
    s += '\t'; s += f != f ? std::string("NaN") : std::isinf(f) ? std::string("inf") : f32_text(f);
  }
  s += '\t'; s += f64_display(t.map_pvalue[i]); s += '\t'; s += f64_display(t.effect_size[i]);
}

// the rows of sites [from, to)
template <class F32Text> void dmr_sites_rows_text(std::string& s, const mkp_dmr_sites_out& t, const char* const* contig_names, uint64_t from, uint64_t to,
    F32Text f32_text) {
  for (uint64_t i = from; i < to; i++) { dmr_sites_row_text(s, t, contig_names, i, f32_text); s += '\n'; }
}

}  // namespace mkp
