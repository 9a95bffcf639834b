// The f32 arithmetic `modkit dmr pair` without -r adds for replicates (src/dmr/single_site.rs: collapse_counts(_, true) and the pct_*_samples of
// SingleSiteDmrScore::new_multi), once for the kernel (mkp_dmr_reps.hip), the host (mkp_host_dmr_reps_balance) and tests/dmr_reps_math_host.cpp.
// HIP-free, `__host__ __device__` by the macro of mkp_dmr_site_math.hpp.  Every step is one correctly rounded f32 operation (the build forbids
// fast-math and contraction); Rust's `as usize` of an f32 saturates and turns NaN into 0: both are written out, no NaN is ever cast.
#pragma once
#include "mkp_dmr_site_math.hpp"

namespace mkp {

// `x as usize` for an f32 that is already whole (or NaN, or infinite)
MKP_SM_HD uint64_t dmr_reps_f32_to_count(float x) {
  if (x != x || x <= 0.0f) return 0;
  if (x >= 18446744073709551616.0f) return 0xffffffffffffffffull;
  return (uint64_t)x;
}

// floor((n_present as f32 / n as f32) * 100f32): the share of a side's samples that hold a site
MKP_SM_HD uint32_t dmr_reps_pct_samples(uint32_t n_present, uint32_t n) {
  return (uint32_t)dmr_reps_f32_to_count(::floorf(((float)n_present / (float)n) * 100.0f));
}

// target_cov of a side: the summed totals of its present samples over their number
MKP_SM_HD float dmr_reps_target(uint64_t sum_total, uint32_t n_present) { return (float)sum_total / (float)n_present; }

// one code of one present sample: floor((count / total) * target); 0 / 0 is NaN in the reference and its cast 0
MKP_SM_HD uint64_t dmr_reps_balanced_count(uint64_t count, uint64_t total, float target) {
  const float frac = (float)count / (float)total;
  if (frac != frac) return 0;
  const float v = frac * target;
  if (v != v) return 0;
  return dmr_reps_f32_to_count(::floorf(v));
}

// a present sample's balanced total: `target_cov as usize` (truncation)
MKP_SM_HD uint64_t dmr_reps_balanced_total(float target) { return dmr_reps_f32_to_count(::truncf(target)); }

// One side of one site: n samples hold it, sample s has counts mod[s * n_codes + k] for the columns of has[s] and the total total[s].
// out_mod[k] / *out_has / *out_total = collapse_counts(_, true).  false: a sample's balanced counts sum beyond its balanced total, where the
// reference aborts (try_new(..).unwrap()): the site counts as a model failure.  T = uint32_t or uint64_t.
template <class T> MKP_SM_HD bool dmr_reps_balance(const T* mod, const uint32_t* has, const T* total, uint32_t n, uint32_t n_codes, uint64_t* out_mod,
    uint32_t* out_has, uint64_t* out_total) {
  for (uint32_t k = 0; k < n_codes; k++) out_mod[k] = 0;
  *out_has = 0; *out_total = 0;
  if (n == 1u) {
    for (uint32_t k = 0; k < n_codes; k++) if ((has[0] >> k) & 1u) out_mod[k] = mod[k];
    *out_has = has[0]; *out_total = total[0];
    return true;
  }
  uint64_t sum = 0;
  for (uint32_t s = 0; s < n; s++) sum += total[s];
  const float target = dmr_reps_target(sum, n);
  const uint64_t each = dmr_reps_balanced_total(target);
  bool ok = true;
  for (uint32_t s = 0; s < n; s++) {
    uint64_t m = 0;
    for (uint32_t k = 0; k < n_codes; k++) if ((has[s] >> k) & 1u) {
      const uint64_t c = dmr_reps_balanced_count(mod[(size_t)s * n_codes + k], total[s], target);
      out_mod[k] += c; m += c;
    }
    if (m > each) ok = false;
    *out_has |= has[s]; *out_total += each;
  }
  return ok;
}

}  // namespace mkp
