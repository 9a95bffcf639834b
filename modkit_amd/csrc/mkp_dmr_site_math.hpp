// The arithmetic of one site of `modkit dmr pair` without -r (src/dmr/llr_model.rs:227-330, beta_diff.rs), once for the kernel
// (mkp_dmr_sites.hip) and the host (mkp_host_dmr_site_score, tests/dmr_site_math_host.cpp): the likelihood-ratio score over per-code counts and
// the MAP-based p-value of PMapEstimator::run.  HIP-free: fixed arrays, no allocation, `__host__ __device__` by macro as mkp_bedmethyl_line.hpp.
// IEEE values flow as in the reference: a total of 0 gives NaN for p and effect, an overflowing quadrature gives ln_effect = inf and p = 0.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MKP_SM_HD __host__ __device__ __forceinline__
#define MKP_SM_MEMBER __host__ __device__ __forceinline__
#define MKP_SM_UNROLL _Pragma("unroll")   // (the kernel keeps the count arrays in registers: every index is a constant once unrolled)
#else
#define MKP_SM_HD static inline
#define MKP_SM_MEMBER inline
#define MKP_SM_UNROLL
#endif

#define MKP_DMR_SITE_MAX_CODES 16   // code columns of a site (MKP_STATS_MAX_CODES)
#define MKP_DMR_SITE_GL 16          // Gauss-Legendre points of appell_f1_stable
#define MKP_DMR_SITE_MAX_COV 300u   // MAX_COV_ALLOWED

// prior Beta(alpha, beta), rope = --delta, max_cov = the two max coverages (already capped at MKP_DMR_SITE_MAX_COV), and the quadrature's
// nodes (ascending) and weights on [-1, 1]
struct MkpDmrSiteMath { double alpha, beta, delta; uint32_t max_cov[2]; double gl_x[MKP_DMR_SITE_GL], gl_w[MKP_DMR_SITE_GL]; };

namespace mkp {

// one vector of llk (mkp_dmr.hpp's dmr_llk), fed a category at a time in the order dmr_llk walks it
struct DmrLlkAcc {
  double N = 0, twice = 0, once = 0;
  MKP_SM_MEMBER void add(uint64_t v) { const double x = (double)v; N += x; twice += ::lgamma(0.5 + 2.0 * x); once += ::lgamma(0.5 + x); }
  MKP_SM_MEMBER double done(uint32_t k) const { const double k2 = 0.5 * (double)k; return (twice - ::lgamma(k2 + 2.0 * N)) - (once - ::lgamma(k2 + N)); }
};

// llk_ratio over n_codes code columns (ascending code): bit k of a_has / b_has = the sample's key set holds column k, a_mod[k] its count.
// false: the reference fails (one code against a different code; counts beyond the total).  T = uint32_t or uint64_t.
template <class T> MKP_SM_HD bool dmr_site_llk_ratio(const T* a_mod, uint32_t a_has, uint64_t a_total, const T* b_mod, uint32_t b_has, uint64_t b_total,
    uint32_t n_codes, double* score) {
  uint32_t ka = 0, kb = 0, ku = 0; uint64_t sa = 0, sb = 0;
  MKP_SM_UNROLL
  for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) if (k < n_codes) {
    if ((a_has >> k) & 1u) { ka++; sa += a_mod[k]; }
    if ((b_has >> k) & 1u) { kb++; sb += b_mod[k]; }
    if (((a_has | b_has) >> k) & 1u) ku++;
  }
  *score = 0.0;
  if (sa > a_total || sb > b_total) return false;   // AggregatedCounts::try_new
  const uint32_t n_categories = (ka > kb ? ka : kb) + 1u;
  if (n_categories < 2u) return true;
  if (n_categories == 2u && ku != 1u) return false;   // llk_beta: "should have exactly one modification"
  DmrLlkAcc a, b, ab;
  a.add(a_total - sa); b.add(b_total - sb); ab.add(a_total - sa + (b_total - sb));
  MKP_SM_UNROLL
  for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) if (k < n_codes && (((a_has | b_has) >> k) & 1u)) {
    const uint64_t x = ((a_has >> k) & 1u) ? (uint64_t)a_mod[k] : 0, y = ((b_has >> k) & 1u) ? (uint64_t)b_mod[k] : 0;
    a.add(x); b.add(y); ab.add(x + y);
  }
  *score = a.done(ku + 1u) + b.done(ku + 1u) - ab.done(ku + 1u);
  return true;
}

MKP_SM_HD double dmr_ln_beta(double a, double b) { return ::lgamma(a) + ::lgamma(b) - ::lgamma(a + b); }

// PMapEstimator::run over Counts{n_mod, coverage}.  false: the reference fails (n_mod beyond the coverage; the null's parameter sums below 1).
// ln_effect / ln_null are NaN where the reference does not compute them (the p = 1 shortcuts).
MKP_SM_HD bool dmr_site_pmap(const MkpDmrSiteMath& M, uint64_t a_mod, uint64_t a_cov, uint64_t b_mod, uint64_t b_cov, double* ln_effect_out,
    double* ln_null_out, double* p_out, double* effect_out) {
  const double nan = __builtin_nan("");
  *ln_effect_out = nan; *ln_null_out = nan; *p_out = nan; *effect_out = nan;
  if (a_mod > a_cov || b_mod > b_cov) return false;   // Counts::new
  double fa = (double)a_mod / (double)a_cov, fb = (double)b_mod / (double)b_cov;
  // resize: Rust's f64::round is C's round (half away from zero)
  if (a_cov > M.max_cov[0]) { const double m = (double)M.max_cov[0], n = ::round(fa * m); fa = n / m; a_mod = (uint64_t)n; a_cov = M.max_cov[0]; }
  if (b_cov > M.max_cov[1]) { const double m = (double)M.max_cov[1], n = ::round(fb * m); fb = n / m; b_mod = (uint64_t)n; b_cov = M.max_cov[1]; }
  const double e = fa - fb;
  *effect_out = e;
  if (::fabs(e) <= M.delta) { *p_out = 1.0; return true; }
  const double d = e > 0.0 ? e - 0.005 : e + 0.005;
  const double a1 = M.alpha + (double)a_mod, b1 = M.beta + (double)(a_cov - a_mod), a2 = M.alpha + (double)b_mod, b2 = M.beta + (double)(b_cov - b_mod);
  const double ln_A = dmr_ln_beta(a1, b1) + dmr_ln_beta(a2, b2);
  const bool null_ok = !(a1 + a2 < 1.0 || b1 + b2 < 1.0);
  double ln_effect;
  if (::fabs(d) < M.delta) {   // calc_beta_diff's first branch (an |e| just above delta)
    if (!null_ok) return false;
    ln_effect = dmr_ln_beta(a1 + a2 - 1.0, b1 + b2 - 1.0) - ln_A;
  } else {
    // the two long branches differ in their parameters only: select them, then one quadrature for both
    const bool up = d > 0.0;
    const double all = a1 + b1 + a2 + b2 - 2.0;
    const double x = up ? 1.0 - d : 1.0 - d * d, y = up ? 1.0 - d * d : 1.0 + d;
    const double a = up ? b1 : b2, q1 = up ? all : 1.0 - a2, q2 = up ? 1.0 - a1 : all, c = up ? a2 + b1 : a1 + b2;
    const double lb = up ? dmr_ln_beta(a2, b1) : dmr_ln_beta(a1, b2);
    const double t1 = ::log(up ? d : -d) * (b1 + b2 - 1.0), t2 = ::log(up ? 1.0 - d : 1.0 + d) * (c - 1.0);
    const double lower = 1e-5, upper = 1.0 - 1e-5, half_diff = (upper - lower) / 2.0, half_sum = (lower + upper) / 2.0;
    double sum = 0.0;
    for (int i = 0; i < MKP_DMR_SITE_GL; i++) {
      const double u = half_diff * M.gl_x[i] + half_sum;
      const double numer = (a - 1.0) * ::log(u) + (-a + c - 1.0) * ::log(1.0 - u);
      const double denom = q1 * ::log(1.0 - u * x) + q2 * ::log(1.0 - y * u);
      sum += M.gl_w[i] * ::exp(numer - denom);
    }
    const double f1 = ::log(half_diff * sum) - dmr_ln_beta(a, c - a);
    ln_effect = lb + t1 + t2 + f1 - ln_A;
  }
  *ln_effect_out = ln_effect;
  if (::exp(ln_effect) == 0.0) { *p_out = 1.0; return true; }
  if (!null_ok) return false;
  const double ln_null = dmr_ln_beta(a1 + a2 - 1.0, b1 + b2 - 1.0) - ln_A;
  *ln_null_out = ln_null;
  const double p = ::exp(ln_null - ln_effect);
  *p_out = p > 1.0 ? 1.0 : p;
  return true;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The 16 Gauss-Legendre nodes (ascending) and weights on [-1, 1]: Newton's iteration on P_16 from the Chebyshev guess
static inline void dmr_gauss_legendre(double* x, double* w) {
  const int n = MKP_DMR_SITE_GL;
  for (int i = 0; i < n / 2; i++) {
    double z = ::cos(3.14159265358979323846 * ((double)i + 0.75) / ((double)n + 0.5)), dp = 0.0;
    for (int it = 0; it < 100; it++) {
      double p0 = 1.0, p1 = z;
      for (int k = 2; k <= n; k++) { const double p2 = ((2.0 * k - 1.0) * z * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = p2; }
      dp = n * (z * p1 - p0) / (z * z - 1.0);
      const double dz = p1 / dp;
      z -= dz;
      if (::fabs(dz) < 1e-16) break;
    }
    {   // the derivative at the converged root
      double p0 = 1.0, p1 = z;
      for (int k = 2; k <= n; k++) { const double p2 = ((2.0 * k - 1.0) * z * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = p2; }
      dp = n * (z * p1 - p0) / (z * z - 1.0);
    }
    const double wt = 2.0 / ((1.0 - z * z) * dp * dp);
    x[i] = -z; x[n - 1 - i] = z; w[i] = wt; w[n - 1 - i] = wt;
  }
}
#endif

}  // namespace mkp
