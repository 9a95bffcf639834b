// `modkit dmr pair` without -r (src/dmr/single_site.rs, beta_diff.rs, llr_model.rs) over bedMethyl rows that are already in HBM: the two
// tables are compared position by position, and every site both hold gets the likelihood-ratio score and the MAP-based p-value, in f64, one
// lane a site.  The arithmetic is mkp_dmr_site_math.hpp's, the row filter mkp_dev_dmr_filter.hpp's (a '.' rule over the whole contig).
//
// Input per (sample, contig): six SoA row columns, ascending in `pos`, whole (the host joins the pieces, so no position is cut), and the
// contig's reference bytes [0, ref_len).  Stages, in the order the host runs them (mkp_dmr_sites_get):
//   listed     per window of `interval` bp the number of positions get_positions lists: what the host's batch planner walks
//   flags      a lane a row: does it take part, its code slot (resolve_slot), is it the head of its position; per tile of 256 rows the number
//              of heads and of participating rows
//   scan       one workgroup: exclusive scan of the tile counts, and the totals
//   heads      a lane a row: the head of a position gets its site index from the tile's offset and a ballot rank, walks its group (one to a few
//              rows) and writes the site: pos, first row, total, strand, and the bad bit where the group disagrees on N_valid_cov or
//              N_canonical or N_canonical + sum N_mod != N_valid_cov
//   bounds     per batch-table entry the number of participating rows in front of its start (the estimate of the max coverages)
//   coverages  the N_valid_cov of the participating rows in front of a row, compacted in no particular order (they are sorted next)
//   bad        every bad site marks its batch, for both samples, before the join
//   join       a lane an `a` site: binary search of b's sorted keys; kept when b holds it and its batch is not marked; tile counts, scan, pairs
//   score      a lane a pair: walks both groups' rows, sums N_mod per code column, then llk_ratio and the p-value
#include "mkp_dev_codeslots.hpp"
#include "mkp_dev_dmr_filter.hpp"
#include "mkp_dev_dmr_sites.hpp"
#include "mkp_dmr_site_math.hpp"
#include "mkp_launch.h"

namespace {

constexpr uint32_t kTile = MKP_DMRS_TILE;

__global__ __launch_bounds__(256) void mkp_dmr_sites_listed(const uint8_t* __restrict__ ref, uint32_t ref_len, unsigned long long interval,
    uint32_t n_windows, const MkpDmrParams P, uint32_t* __restrict__ counts) {
  __shared__ uint32_t sh[4];
  for (uint32_t w = blockIdx.x; w < n_windows; w += gridDim.x) {
    const unsigned long long from = (unsigned long long)w * interval, to = min(from + interval, (unsigned long long)ref_len);
    uint32_t mine = 0;
    for (unsigned long long i = from + threadIdx.x; i < to; i += blockDim.x)
      mine += listed_strand(P, base_index(ref[i], P.mask != 0u), 3u) < 2u ? 1u : 0u;
    mine = wave_incl_scan(mine);
    if (lane_id() == 63) sh[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) counts[w] = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void mkp_dmr_sites_flags(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ info,
    const uint32_t* __restrict__ code, const uint32_t* __restrict__ n_valid, uint32_t n_rows, const uint8_t* __restrict__ ref, uint32_t ref_len,
    const MkpDmrParams P, uint32_t* codes, uint32_t* err, uint8_t* __restrict__ rowflag, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t sh[4];
  const int lane = lane_id();
  const uint32_t i = blockIdx.x * kTile + threadIdx.x;
  uint32_t tab = load_codes(codes, lane);
  bool part = false, head = false; uint32_t c = 0;
  if (i < n_rows) {
    const uint32_t p = pos[i];
    c = code[i];
    const uint32_t bidx = p < ref_len ? base_index(ref[p], P.mask != 0u) : 4u, listed = listed_strand(P, bidx, 3u);
    part = takes_part(P, bidx, listed, info[i] & 3u, c, n_valid[i]);
    head = part;
    for (uint32_t j = i; head && j > 0 && pos[j - 1] == p; j--)
      if (takes_part(P, bidx, listed, info[j - 1] & 3u, code[j - 1], n_valid[j - 1])) head = false;
  }
  const int slot = resolve_slot(tab, codes, err, part, c, true, lane);   // (every lane of the wave)
  if (i < n_rows) rowflag[i] = (uint8_t)(part ? ((slot >= 0 ? (uint32_t)slot : 0u) | MKP_DMRS_ROW_PART | (head ? MKP_DMRS_ROW_HEAD : 0u)) : 0u);
  uint32_t n_heads = 0, n_part = 0;
  (void)block_rank(head, sh, &n_heads);
  (void)block_rank(part, sh, &n_part);
  if (threadIdx.x == 0) { tile_cnt[2 * blockIdx.x] = n_heads; tile_cnt[2 * blockIdx.x + 1] = n_part; }
}

// cnt[2 t], cnt[2 t + 1]: two counters per tile -> their exclusive prefixes; totals[0 .. 2): the sums.  One workgroup of 1024.
__global__ __launch_bounds__(1024) void mkp_dmr_sites_scan(uint32_t* __restrict__ cnt, uint32_t n_tiles, uint32_t* __restrict__ totals) {
  __shared__ uint32_t sum[2][1024];
  const uint32_t per = (n_tiles + 1023u) / 1024u, first = min(threadIdx.x * per, n_tiles), last = min(first + per, n_tiles);
  uint32_t a = 0, b = 0;
  for (uint32_t t = first; t < last; t++) { a += cnt[2 * t]; b += cnt[2 * t + 1]; }
  sum[0][threadIdx.x] = a; sum[1][threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x < 2) {   // (1024 additions a counter)
    uint32_t run = 0;
    for (uint32_t k = 0; k < 1024u; k++) { const uint32_t v = sum[threadIdx.x][k]; sum[threadIdx.x][k] = run; run += v; }
    totals[threadIdx.x] = run;
  }
  __syncthreads();
  a = sum[0][threadIdx.x]; b = sum[1][threadIdx.x];
  for (uint32_t t = first; t < last; t++) { const uint32_t x = cnt[2 * t], y = cnt[2 * t + 1]; cnt[2 * t] = a; cnt[2 * t + 1] = b; a += x; b += y; }
}

__global__ __launch_bounds__(256) void mkp_dmr_sites_heads(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ info,
    const uint32_t* __restrict__ n_valid, const uint32_t* __restrict__ n_mod, const uint32_t* __restrict__ n_can, const uint8_t* __restrict__ rowflag,
    uint32_t n_rows, const uint32_t* __restrict__ tile_off, uint32_t* __restrict__ s_pos, uint32_t* __restrict__ s_first,
    uint32_t* __restrict__ s_total, uint32_t* __restrict__ s_info) {
  __shared__ uint32_t sh[4];
  const uint32_t i = blockIdx.x * kTile + threadIdx.x;
  const bool head = i < n_rows && (rowflag[i] & MKP_DMRS_ROW_HEAD);
  uint32_t all = 0;
  const uint32_t site = tile_off[2 * blockIdx.x] + block_rank(head, sh, &all);
  if (!head) return;
  const uint32_t p = pos[i], g_nv = n_valid[i], g_nc = n_can[i];
  unsigned long long g_mod = 0; bool bad = false;
  for (uint32_t j = i; j < n_rows && pos[j] == p; j++) {
    if (!(rowflag[j] & MKP_DMRS_ROW_PART)) continue;
    g_mod += n_mod[j];
    if (n_valid[j] != g_nv || n_can[j] != g_nc) bad = true;
  }
  if ((unsigned long long)g_nc + g_mod != (unsigned long long)g_nv) bad = true;
  s_pos[site] = p; s_first[site] = i; s_total[site] = g_nv;
  s_info[site] = ((info[i] & 3u) == 1u ? MKP_DMRS_SITE_MINUS : 0u) | (bad ? MKP_DMRS_SITE_BAD : 0u);
}

__global__ __launch_bounds__(256) void mkp_dmr_sites_bounds(const uint32_t* __restrict__ pos, const uint8_t* __restrict__ rowflag, uint32_t n_rows,
    const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ totals, const MkpDmrSitesBatch* __restrict__ batches, uint32_t n_entries,
    uint32_t* __restrict__ row_at, uint32_t* __restrict__ part_before) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_entries) return;
  const uint32_t r = lower_bound_u32(pos, n_rows, batches[e].start);
  uint32_t n = totals[1];
  if (r < n_rows) {
    const uint32_t t = r / kTile;
    n = tile_off[2 * t + 1];
    for (uint32_t j = t * kTile; j < r; j++) n += (rowflag[j] & MKP_DMRS_ROW_PART) ? 1u : 0u;
  }
  row_at[e] = r; part_before[e] = n;
}

__global__ __launch_bounds__(256) void mkp_dmr_sites_coverages(const uint8_t* __restrict__ rowflag, const uint32_t* __restrict__ n_valid, uint32_t n_front,
    uint32_t* cursor, uint32_t* __restrict__ out, uint32_t cap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_front || !(rowflag[i] & MKP_DMRS_ROW_PART)) return;
  const uint32_t at = atomicAdd(cursor, 1u);
  if (at < cap) out[at] = n_valid[i];
}

__global__ __launch_bounds__(256) void mkp_dmr_sites_bad(const uint32_t* __restrict__ s_pos, const uint32_t* __restrict__ s_info, uint32_t n_sites,
    const MkpDmrSitesBatch* __restrict__ batches, uint32_t n_entries, uint32_t* bad_batch) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sites || !(s_info[i] & MKP_DMRS_SITE_BAD)) return;
  atomicOr(&bad_batch[batches[batch_entry(batches, n_entries, s_pos[i])].batch], 1u);
}

__global__ __launch_bounds__(256) void mkp_dmr_sites_join(const uint32_t* __restrict__ a_pos, uint32_t n_a, const uint32_t* __restrict__ b_pos, uint32_t n_b,
    const MkpDmrSitesBatch* __restrict__ batches, uint32_t n_entries, const uint32_t* __restrict__ bad_batch, uint32_t* __restrict__ partner,
    uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t sh[4];
  const uint32_t i = blockIdx.x * kTile + threadIdx.x;
  uint32_t j = MKP_DMRS_NO_PAIR;
  if (i < n_a) {
    const uint32_t p = a_pos[i], at = lower_bound_u32(b_pos, n_b, p);
    if (at < n_b && b_pos[at] == p && !bad_batch[batches[batch_entry(batches, n_entries, p)].batch]) j = at;
    partner[i] = j;
  }
  uint32_t all = 0;
  (void)block_rank(j != MKP_DMRS_NO_PAIR, sh, &all);
  if (threadIdx.x == 0) { tile_cnt[2 * blockIdx.x] = all; tile_cnt[2 * blockIdx.x + 1] = 0; }
}

__global__ __launch_bounds__(256) void mkp_dmr_sites_pairs(const uint32_t* __restrict__ partner, uint32_t n_a, const uint32_t* __restrict__ tile_off,
    uint32_t* __restrict__ pair_a, uint32_t* __restrict__ pair_b) {
  __shared__ uint32_t sh[4];
  const uint32_t i = blockIdx.x * kTile + threadIdx.x;
  const uint32_t j = i < n_a ? partner[i] : MKP_DMRS_NO_PAIR;
  uint32_t all = 0;
  const uint32_t at = tile_off[2 * blockIdx.x] + block_rank(j != MKP_DMRS_NO_PAIR, sh, &all);
  if (j != MKP_DMRS_NO_PAIR) { pair_a[at] = i; pair_b[at] = j; }
}

__global__ __launch_bounds__(256) void mkp_dmr_sites_score(const MkpDmrSitesSample A, const MkpDmrSitesSample B, const uint32_t* __restrict__ pair_a,
    const uint32_t* __restrict__ pair_b, uint32_t n_pairs, unsigned long long col_of_slot, uint32_t n_cols, const MkpDmrSiteMath M,
    const MkpDmrSitesPairs out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  const uint32_t ia = pair_a[i], ib = pair_b[i];
  uint32_t ca[MKP_DMR_SITE_MAX_CODES], cb[MKP_DMR_SITE_MAX_CODES], ha = 0, hb = 0;
#pragma unroll
  for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) { ca[k] = 0; cb[k] = 0; }
  sum_group(A, ia, col_of_slot, ca, &ha);
  sum_group(B, ib, col_of_slot, cb, &hb);
  const uint32_t ta = A.s_total[ia], tb = B.s_total[ib];
  unsigned long long ma = 0, mb = 0;
#pragma unroll
  for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) { ma += ca[k]; mb += cb[k]; }
  // PMapEstimator::predict comes first in SingleSiteDmrScore::new_multi, then llk_ratio: either failing fails the site
  double ln_effect, ln_null, p, effect, score = 0.0;
  bool ok = mkp::dmr_site_pmap(M, ma, ta, mb, tb, &ln_effect, &ln_null, &p, &effect);
  ok = mkp::dmr_site_llk_ratio<uint32_t>(ca, ha, ta, cb, hb, tb, n_cols, &score) && ok;
  out.pos[i] = A.s_pos[ia];
  out.info[i] = (A.s_info[ia] & MKP_DMRS_SITE_MINUS) | (ok ? 0u : MKP_DMRS_PAIR_FAILED);
  out.has[i] = ha | (hb << 16);
  out.total_a[i] = ta; out.total_b[i] = tb;
  uint32_t* cnt = out.cnt + (size_t)i * 2u * n_cols;
#pragma unroll
  for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) if (k < n_cols) { cnt[k] = ca[k]; cnt[n_cols + k] = cb[k]; }
  out.score[i] = score; out.pvalue[i] = p; out.effect[i] = effect;
}

uint32_t tiles_of(uint32_t n) { return (n + kTile - 1u) / kTile; }

}  // namespace

extern "C" hipError_t mkp_launch_dmr_sites_listed(hipStream_t st, const uint8_t* ref, uint32_t ref_len, unsigned long long interval, uint32_t n_windows,
    const MkpDmrParams* prm, uint32_t* counts) {
  if (!n_windows) return hipSuccess;
  mkp_dmr_sites_listed<<<std::min(n_windows, 4096u), 256, 0, st>>>(ref, ref_len, interval, n_windows, *prm, counts);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_sites_heads(hipStream_t st, const uint32_t* pos, const uint32_t* info, const uint32_t* code, const uint32_t* n_valid,
    const uint32_t* n_mod, const uint32_t* n_can, uint32_t n_rows, const uint8_t* ref, uint32_t ref_len, const MkpDmrParams* prm, uint32_t* codes,
    uint32_t* err, uint8_t* rowflag, uint32_t* tile_cnt, uint32_t* totals, uint32_t* s_pos, uint32_t* s_first, uint32_t* s_total, uint32_t* s_info) {
  if (!n_rows) return hipMemsetAsync(totals, 0, 8, st);
  const uint32_t n_tiles = tiles_of(n_rows);
  mkp_dmr_sites_flags<<<n_tiles, 256, 0, st>>>(pos, info, code, n_valid, n_rows, ref, ref_len, *prm, codes, err, rowflag, tile_cnt);
  mkp_dmr_sites_scan<<<1, 1024, 0, st>>>(tile_cnt, n_tiles, totals);
  mkp_dmr_sites_heads<<<n_tiles, 256, 0, st>>>(pos, info, n_valid, n_mod, n_can, rowflag, n_rows, tile_cnt, s_pos, s_first, s_total, s_info);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_sites_scan(hipStream_t st, uint32_t* cnt, uint32_t n_tiles, uint32_t* totals) {
  mkp_dmr_sites_scan<<<1, 1024, 0, st>>>(cnt, n_tiles, totals);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_sites_bounds(hipStream_t st, const uint32_t* pos, const uint8_t* rowflag, uint32_t n_rows, const uint32_t* tile_off,
    const uint32_t* totals, const MkpDmrSitesBatch* batches, uint32_t n_entries, uint32_t* row_at, uint32_t* part_before) {
  if (!n_entries) return hipSuccess;
  mkp_dmr_sites_bounds<<<(n_entries + 255u) / 256u, 256, 0, st>>>(pos, rowflag, n_rows, tile_off, totals, batches, n_entries, row_at, part_before);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_sites_coverages(hipStream_t st, const uint8_t* rowflag, const uint32_t* n_valid, uint32_t n_front, uint32_t* cursor,
    uint32_t* out, uint32_t cap) {
  if (!n_front) return hipSuccess;
  mkp_dmr_sites_coverages<<<(n_front + 255u) / 256u, 256, 0, st>>>(rowflag, n_valid, n_front, cursor, out, cap);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_sites_bad(hipStream_t st, const uint32_t* s_pos, const uint32_t* s_info, uint32_t n_sites,
    const MkpDmrSitesBatch* batches, uint32_t n_entries, uint32_t* bad_batch) {
  if (!n_sites || !n_entries) return hipSuccess;
  mkp_dmr_sites_bad<<<(n_sites + 255u) / 256u, 256, 0, st>>>(s_pos, s_info, n_sites, batches, n_entries, bad_batch);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_sites_join(hipStream_t st, const uint32_t* a_pos, uint32_t n_a, const uint32_t* b_pos, uint32_t n_b,
    const MkpDmrSitesBatch* batches, uint32_t n_entries, const uint32_t* bad_batch, uint32_t* partner, uint32_t* tile_cnt, uint32_t* totals,
    uint32_t* pair_a, uint32_t* pair_b) {
  if (!n_a || !n_entries) return hipMemsetAsync(totals, 0, 8, st);
  const uint32_t n_tiles = tiles_of(n_a);
  mkp_dmr_sites_join<<<n_tiles, 256, 0, st>>>(a_pos, n_a, b_pos, n_b, batches, n_entries, bad_batch, partner, tile_cnt);
  mkp_dmr_sites_scan<<<1, 1024, 0, st>>>(tile_cnt, n_tiles, totals);
  mkp_dmr_sites_pairs<<<n_tiles, 256, 0, st>>>(partner, n_a, tile_cnt, pair_a, pair_b);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dmr_sites_score(hipStream_t st, const MkpDmrSitesSample* a, const MkpDmrSitesSample* b, const uint32_t* pair_a,
    const uint32_t* pair_b, uint32_t n_pairs, unsigned long long col_of_slot, uint32_t n_cols, const MkpDmrSiteMath* math, const MkpDmrSitesPairs* out) {
  if (!n_pairs) return hipSuccess;
  mkp_dmr_sites_score<<<(n_pairs + 255u) / 256u, 256, 0, st>>>(*a, *b, pair_a, pair_b, n_pairs, col_of_slot, n_cols, *math, *out);
  return hipGetLastError();
}
