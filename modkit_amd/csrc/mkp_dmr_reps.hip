// `modkit dmr pair` without -r over replicates (SingleSiteDmrScore::new_multi and collapse_counts, src/dmr/single_site.rs): several `a` and `b`
// tables compared position by position.  Every sample of a contig goes through the stages of mkp_dmr_sites.hip up to its sites and bad batches
// (mkp_launch_dmr_sites_heads / _bad, unchanged); this file joins the sides and scores the joined sites.  Stages, per contig:
//   mark     a lane a site of a sample: its position's bit in the side's bitmap (one bit a contig position, atomicOr)
//   join     a lane a bitmap word: a & b with the positions of dropped batches taken out, written over a's word; per tile of 256 words the
//            number of joined sites
//   scan     mkp_launch_dmr_sites_scan over the tile counts
//   list     a lane a word: its joined positions, ascending, at the tile's offset plus the workgroup's exclusive scan
//   gather   a lane a joined site: binary search of every sample's sites; the present samples' groups summed per code column (sum_group) into
//            the collapsed counts, the balanced counts in f32 (mkp_dmr_reps_math.hpp), the per-sample (modified, total) by rank for the
//            replicate pairs, the presence masks and the shares of samples
//   tasks    the evaluations of every joined site flattened into two task lists (count, mkp_launch_dmr_sites_scan, first task per site): a
//            site has its replicate pairs by rank, the balanced and the collapsed p-value, and the balanced and the collapsed ratio; a site
//            with one present sample a side has the collapsed pair alone, every other value being the same number
//   score    a lane a p-value task: straight-line, one call of dmr_site_pmap; a failure sets the site's bit (atomicOr)
//   ratio    a lane a ratio task: one call of dmr_site_llk_ratio
#include "mkp_dev_codeslots.hpp"
#include "mkp_dev_dmr_sites.hpp"
#include "mkp_dmr_reps_math.hpp"
#include "mkp_launch.h"

namespace {

constexpr uint32_t kTile = MKP_DMRS_TILE;

// the sum of v over the workgroup's lanes in front of this one, and (in *total) over all of them; sh: 4 words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const uint32_t incl = wave_incl_scan(v), wave = threadIdx.x >> 6;
  if (lane_id() == 63) sh[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < (blockDim.x >> 6); w++) { const uint32_t x = sh[w]; if (w < wave) before += x; all += x; }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

__global__ __launch_bounds__(256) void mkp_dmr_reps_mark(const uint32_t* __restrict__ s_pos, uint32_t n_sites, uint32_t* bits, uint32_t n_words) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sites) return;
  const uint32_t p = s_pos[i];
  if ((p >> 5) < n_words) atomicOr(&bits[p >> 5], 1u << (p & 31u));
}

__global__ __launch_bounds__(256) void mkp_dmr_reps_join(uint32_t* __restrict__ a_bits, const uint32_t* __restrict__ b_bits, uint32_t n_words,
    const MkpDmrSitesBatch* __restrict__ batches, uint32_t n_entries, const uint32_t* __restrict__ bad_batch, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t sh[4];
  const uint32_t w = blockIdx.x * kTile + threadIdx.x;
  uint32_t v = 0;
  if (w < n_words) {
    v = a_bits[w] & b_bits[w];
    if (v) {
      const uint32_t e0 = batch_entry(batches, n_entries, w * 32u), e1 = batch_entry(batches, n_entries, w * 32u + 31u);
      if (e0 == e1) { if (bad_batch[batches[e0].batch]) v = 0; }
      else for (uint32_t m = v; m; m &= m - 1u) {   // (a batch begins inside the word)
        const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
        if (bad_batch[batches[batch_entry(batches, n_entries, w * 32u + bit)].batch]) v &= ~(1u << bit);
      }
    }
    a_bits[w] = v;
  }
  uint32_t all = 0;
  (void)block_excl_scan((uint32_t)__popc(v), sh, &all);
  if (threadIdx.x == 0) { tile_cnt[2 * blockIdx.x] = all; tile_cnt[2 * blockIdx.x + 1] = 0; }
}

__global__ __launch_bounds__(256) void mkp_dmr_reps_list(const uint32_t* __restrict__ bits, uint32_t n_words, const uint32_t* __restrict__ tile_off,
    uint32_t* __restrict__ j_pos, uint32_t n_joined) {
  __shared__ uint32_t sh[4];
  const uint32_t w = blockIdx.x * kTile + threadIdx.x;
  const uint32_t v = w < n_words ? bits[w] : 0u;
  uint32_t all = 0;
  uint32_t at = tile_off[2 * blockIdx.x] + block_excl_scan((uint32_t)__popc(v), sh, &all);
  for (uint32_t m = v; m; m &= m - 1u, at++) if (at < n_joined) j_pos[at] = w * 32u + (uint32_t)__ffs((int)m) - 1u;
}

// the site of sample S at position p, or MKP_DMRS_NO_PAIR
__device__ __forceinline__ uint32_t site_at(const MkpDmrRepsSample& S, uint32_t p) {
  const uint32_t at = lower_bound_u32(S.s.s_pos, S.n_sites, p);
  return at < S.n_sites && S.s.s_pos[at] == p ? at : MKP_DMRS_NO_PAIR;
}

__global__ __launch_bounds__(256) void mkp_dmr_reps_gather(const MkpDmrRepsSample* __restrict__ samples, uint32_t n_a, uint32_t n_b,
    const uint32_t* __restrict__ j_pos, uint32_t n_joined, unsigned long long col_of_slot, uint32_t n_cols, uint32_t rep_stride, const MkpDmrRepsSites out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_joined) return;
  const uint32_t p = j_pos[i];
  uint32_t info = 0, present = 0, pct = 0, has_both = 0;
  for (uint32_t side = 0; side < 2u; side++) {
    const uint32_t n = side ? n_b : n_a;
    const MkpDmrRepsSample* __restrict__ S = samples + (side ? n_a : 0u);
    // the present samples and their summed totals, then their groups
    uint32_t mask = 0; unsigned long long sum = 0;
    for (uint32_t s = 0; s < n; s++) {
      const uint32_t at = site_at(S[s], p);
      if (at == MKP_DMRS_NO_PAIR) continue;
      mask |= 1u << s; sum += S[s].s.s_total[at]; info |= S[s].s.s_info[at] & MKP_DMRS_SITE_MINUS;
    }
    const uint32_t n_present = (uint32_t)__popc(mask);
    const float target = mkp::dmr_reps_target(sum, n_present);
    const unsigned long long each = mkp::dmr_reps_balanced_total(target);
    uint32_t cc[MKP_DMR_SITE_MAX_CODES], bc[MKP_DMR_SITE_MAX_CODES], has = 0, rank = 0;
    unsigned long long m_col = 0, m_bal = 0;
#pragma unroll
    for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) { cc[k] = 0; bc[k] = 0; }
    for (uint32_t s = 0; s < n; s++) {
      if (!((mask >> s) & 1u)) continue;
      const uint32_t at = site_at(S[s], p), t = S[s].s.s_total[at];
      uint32_t cs[MKP_DMR_SITE_MAX_CODES], hs = 0;
#pragma unroll
      for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) cs[k] = 0;
      sum_group(S[s].s, at, col_of_slot, cs, &hs);
      unsigned long long ms = 0, mbs = 0;
#pragma unroll
      for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) {
        const uint32_t b = n_present == 1u ? cs[k] : ((hs >> k) & 1u) ? (uint32_t)mkp::dmr_reps_balanced_count(cs[k], t, target) : 0u;
        cc[k] += cs[k]; bc[k] += b; ms += cs[k]; mbs += b;
      }
      if (n_present > 1u && mbs > each) info |= MKP_DMRS_PAIR_FAILED;   // where the reference aborts
      if (rep_stride) { uint32_t* r = out.rep + (((size_t)i * 2u + side) * rep_stride + rank) * 2u; r[0] = (uint32_t)ms; r[1] = t; }
      has |= hs; m_col += ms; m_bal += mbs; rank++;
    }
    const unsigned long long bal_total = n_present == 1u ? sum : each * n_present;
    if (sum > 0xffffffffull || m_col > 0xffffffffull) info |= MKP_DMRR_SITE_OVERFLOW;
    out.total[(size_t)i * 2u + side] = (uint32_t)sum; out.bal_total[(size_t)i * 2u + side] = (uint32_t)bal_total;
    out.msum[(size_t)i * 4u + side] = (uint32_t)m_col; out.msum[(size_t)i * 4u + 2u + side] = (uint32_t)m_bal;
    uint32_t* cnt = out.cnt + ((size_t)i * 2u + side) * n_cols;
    uint32_t* bal = out.bal_cnt + ((size_t)i * 2u + side) * n_cols;
#pragma unroll
    for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) if (k < n_cols) { cnt[k] = cc[k]; bal[k] = bc[k]; }
    present |= mask << (16u * side); has_both |= has << (16u * side);
    pct |= mkp::dmr_reps_pct_samples(n_present, n) << (16u * side);
  }
  out.pos[i] = p; out.info[i] = info; out.present[i] = present; out.pct[i] = pct; out.has[i] = has_both;
}

// the evaluations of a joined site: p-value tasks (the replicate pairs by rank, balanced, collapsed) and ratio tasks (balanced, collapsed); a
// site with one present sample a side has one of each, the collapsed one, every other value being the same number
__device__ __forceinline__ void site_tasks(uint32_t present, uint32_t rep_stride, uint32_t* n_rep, bool* single, uint32_t* n_pmap, uint32_t* n_ratio) {
  const uint32_t pa = (uint32_t)__popc(present & 0xffffu), pb = (uint32_t)__popc(present >> 16);
  *n_rep = rep_stride && pa == pb ? pa : 0u;
  *single = pa == 1u && pb == 1u;
  *n_pmap = *single ? 1u : *n_rep + 2u; *n_ratio = *single ? 1u : 2u;
}

// per tile of 256 joined sites its two task counts; with tile_off (the scanned counts) the second pass writes every site's first tasks
__global__ __launch_bounds__(256) void mkp_dmr_reps_tasks(const uint32_t* __restrict__ present, uint32_t n_joined, uint32_t rep_stride,
    const uint32_t* __restrict__ tile_off, uint32_t* __restrict__ tile_cnt, uint32_t* __restrict__ task_off) {
  __shared__ uint32_t sh[4];
  const uint32_t i = blockIdx.x * kTile + threadIdx.x;
  uint32_t n_rep = 0, n_pmap = 0, n_ratio = 0; bool single = false;
  if (i < n_joined) site_tasks(present[i], rep_stride, &n_rep, &single, &n_pmap, &n_ratio);
  uint32_t all_p = 0, all_r = 0;
  const uint32_t before_p = block_excl_scan(n_pmap, sh, &all_p), before_r = block_excl_scan(n_ratio, sh, &all_r);
  if (!tile_off) { if (threadIdx.x == 0) { tile_cnt[2 * blockIdx.x] = all_p; tile_cnt[2 * blockIdx.x + 1] = all_r; } return; }
  if (i < n_joined) { task_off[2 * i] = tile_off[2 * blockIdx.x] + before_p; task_off[2 * i + 1] = tile_off[2 * blockIdx.x + 1] + before_r; }
}

// the site a task belongs to: the last site whose first task (task_off[2 * site + which]) is not behind it
__device__ __forceinline__ uint32_t task_site(const uint32_t* __restrict__ task_off, uint32_t n_joined, uint32_t which, uint32_t t) {
  uint32_t lo = 0, hi = n_joined;
  while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (task_off[2 * mid + which] <= t) lo = mid; else hi = mid; }
  return lo;
}

// a lane a p-value task: straight-line, ONE call of dmr_site_pmap
__global__ __launch_bounds__(256) void mkp_dmr_reps_score(const uint32_t* __restrict__ task_off, uint32_t n_tasks, uint32_t n_joined, uint32_t rep_stride,
    const MkpDmrSiteMath M, const MkpDmrRepsSites out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tasks) return;
  const uint32_t i = task_site(task_off, n_joined, 0u, t);
  uint32_t n_rep, n_pmap, n_ratio; bool single;
  site_tasks(out.present[i], rep_stride, &n_rep, &single, &n_pmap, &n_ratio);
  const uint32_t e = single ? n_rep + 1u : t - task_off[2 * i];   // [0, n_rep): replicate pairs, n_rep: balanced, n_rep + 1: collapsed
  unsigned long long ma, ta, mb, tb;
  if (e < n_rep) {
    const uint32_t* rep = out.rep + (size_t)i * 4u * rep_stride;
    ma = rep[2u * e]; ta = rep[2u * e + 1u]; mb = rep[2u * (rep_stride + e)]; tb = rep[2u * (rep_stride + e) + 1u];
  } else {
    const uint32_t* tot = (e == n_rep ? out.bal_total : out.total) + (size_t)i * 2u;
    const uint32_t* m = out.msum + (size_t)i * 4u + (e == n_rep ? 2u : 0u);
    ma = m[0]; mb = m[1]; ta = tot[0]; tb = tot[1];
  }
  double ln_effect, ln_null, p, effect;
  if (!mkp::dmr_site_pmap(M, ma, ta, mb, tb, &ln_effect, &ln_null, &p, &effect)) atomicOr(&out.info[i], MKP_DMRS_PAIR_FAILED);
  if (e < n_rep) { out.rep_pvalue[(size_t)i * rep_stride + e] = p; out.rep_effect[(size_t)i * rep_stride + e] = effect; }
  if (e == n_rep || single) { out.bal_pvalue[i] = p; out.bal_effect[i] = effect; }
  if (e == n_rep + 1u) { out.pvalue[i] = p; out.effect[i] = effect; out.n_rep[i] = n_rep; }
  if (single && n_rep) { out.rep_pvalue[(size_t)i * rep_stride] = p; out.rep_effect[(size_t)i * rep_stride] = effect; }
}

// a lane a ratio task: one call of dmr_site_llk_ratio.  The balanced ratio is not written, but its failure is the site's
__global__ __launch_bounds__(256) void mkp_dmr_reps_ratio(const uint32_t* __restrict__ task_off, uint32_t n_tasks, uint32_t n_joined, uint32_t n_cols,
    const MkpDmrRepsSites out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tasks) return;
  const uint32_t i = task_site(task_off, n_joined, 1u, t);
  const uint32_t present = out.present[i];
  const bool single = __popc(present & 0xffffu) == 1 && __popc(present >> 16) == 1;
  const bool collapsed = single || t - task_off[2 * i + 1] == 1u;
  const uint32_t* c = (collapsed ? out.cnt : out.bal_cnt) + (size_t)i * 2u * n_cols;
  const uint32_t* tot = (collapsed ? out.total : out.bal_total) + (size_t)i * 2u;
  uint32_t a[MKP_DMR_SITE_MAX_CODES], b[MKP_DMR_SITE_MAX_CODES];
#pragma unroll
  for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) { a[k] = k < n_cols ? c[k] : 0u; b[k] = k < n_cols ? c[n_cols + k] : 0u; }
  double s = 0.0;
  if (!mkp::dmr_site_llk_ratio<uint32_t>(a, out.has[i] & 0xffffu, tot[0], b, out.has[i] >> 16, tot[1], n_cols, &s)) atomicOr(&out.info[i], MKP_DMRS_PAIR_FAILED);
  if (collapsed) out.score[i] = s;
}

uint32_t tiles_of(uint32_t n) { return (n + kTile - 1u) / kTile; }

}  // namespace

extern "C" hipError_t mkp_launch_dmr_reps_mark(hipStream_t st, const uint32_t* s_pos, uint32_t n_sites, uint32_t* bits, uint32_t n_words) {
  if (!n_sites || !n_words) return hipSuccess;
  mkp_dmr_reps_mark<<<(n_sites + 255u) / 256u, 256, 0, st>>>(s_pos, n_sites, bits, n_words);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_reps_join(hipStream_t st, uint32_t* a_bits, const uint32_t* b_bits, uint32_t n_words,
    const MkpDmrSitesBatch* batches, uint32_t n_entries, const uint32_t* bad_batch, uint32_t* tile_cnt, uint32_t* totals) {
  if (!n_words || !n_entries) return hipMemsetAsync(totals, 0, 8, st);
  const uint32_t n_tiles = tiles_of(n_words);
  mkp_dmr_reps_join<<<n_tiles, 256, 0, st>>>(a_bits, b_bits, n_words, batches, n_entries, bad_batch, tile_cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return mkp_launch_dmr_sites_scan(st, tile_cnt, n_tiles, totals);
}

extern "C" hipError_t mkp_launch_dmr_reps_list(hipStream_t st, const uint32_t* bits, uint32_t n_words, const uint32_t* tile_off, uint32_t* j_pos,
    uint32_t n_joined) {
  if (!n_words || !n_joined) return hipSuccess;
  mkp_dmr_reps_list<<<tiles_of(n_words), 256, 0, st>>>(bits, n_words, tile_off, j_pos, n_joined);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_reps_gather(hipStream_t st, const MkpDmrRepsSample* samples, uint32_t n_a, uint32_t n_b, const uint32_t* j_pos,
    uint32_t n_joined, unsigned long long col_of_slot, uint32_t n_cols, uint32_t rep_stride, const MkpDmrRepsSites* out) {
  if (!n_joined) return hipSuccess;
  mkp_dmr_reps_gather<<<(n_joined + 255u) / 256u, 256, 0, st>>>(samples, n_a, n_b, j_pos, n_joined, col_of_slot, n_cols, rep_stride, *out);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_reps_tasks(hipStream_t st, const uint32_t* present, uint32_t n_joined, uint32_t rep_stride, uint32_t* tile_cnt,
    uint32_t* totals, uint32_t* task_off) {
  if (!n_joined) return hipMemsetAsync(totals, 0, 8, st);
  const uint32_t n_tiles = tiles_of(n_joined);
  mkp_dmr_reps_tasks<<<n_tiles, 256, 0, st>>>(present, n_joined, rep_stride, nullptr, tile_cnt, task_off);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = mkp_launch_dmr_sites_scan(st, tile_cnt, n_tiles, totals);
  if (e != hipSuccess) return e;
  mkp_dmr_reps_tasks<<<n_tiles, 256, 0, st>>>(present, n_joined, rep_stride, tile_cnt, tile_cnt, task_off);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_reps_score(hipStream_t st, const uint32_t* task_off, uint32_t n_pmap_tasks, uint32_t n_ratio_tasks, uint32_t n_joined,
    uint32_t n_cols, uint32_t rep_stride, const MkpDmrSiteMath* math, const MkpDmrRepsSites* out) {
  if (!n_joined) return hipSuccess;
  if (n_pmap_tasks) mkp_dmr_reps_score<<<(n_pmap_tasks + 255u) / 256u, 256, 0, st>>>(task_off, n_pmap_tasks, n_joined, rep_stride, *math, *out);
  if (n_ratio_tasks) mkp_dmr_reps_ratio<<<(n_ratio_tasks + 255u) / 256u, 256, 0, st>>>(task_off, n_ratio_tasks, n_joined, n_cols, *out);
  return hipGetLastError();
}
