// `modkit dmr pair` over regions (src/dmr/pairwise.rs, bedmethyl.rs:172-267, genome_positions.rs:91-127) over bedMethyl rows that are
// already in HBM: per (sample, region) the sum of N_mod per mod code and the total valid coverage over the rows that take part, and
// whether a position of the region is inconsistent.  The score and the text are the host's (mkp_dmr.hpp).
//
// Input: six SoA row columns of one piece of one contig of one sample, ascending in `pos` and cut at a position boundary (pos, info,
// code, n_valid, n_mod, n_canonical: 24 of a row's 44 bytes), the contig's regions and its reference bytes [ref_off, ref_off + ref_len).
// The scheme is that of mkp_stats.hip (mkp_dev_chunks.hpp): bounds, scan, then mkp_dmr_reduce with one wave per (region, 4096-row chunk)
// item on a fixed strided grid, 64 coalesced rows a round.
//
// A row takes part when (a) N_valid_cov >= min_cov, (b) its code is in the code -> base table, (c) the reference base at pos is the
// code's base ('+', '.' rows) or its complement ('-' rows), and (d) get_positions lists that position on the row's strand for the region's
// rule: a base of the positive set is listed '+' where the rule covers '+', and only otherwise may it be listed '-' as a base of the
// negative set.  The reference byte is one gathered byte per row, ascending addresses.
// The rows of one position that take part are a group (aggregate_counts groups by position, strand and base, and a position is listed on
// one strand only).  The lane of a group's first row walks the group, through the chunk's end if need be (a region's rows begin and end
// at position boundaries, so the walk stays inside the region); a row looks backwards over the rows of its position to learn whether it
// is the first; the rows next to it come with the row's own loads.  The walk advances one row per step for all walking lanes at once, so
// that resolve_slot is reached by the whole wave.
// A group must agree on N_valid_cov and N_canonical, and N_canonical + sum N_mod must be N_valid_cov; otherwise the line is marked bad
// (its sums are then never read).  Every row that takes part claims its code's slot, N_mod == 0 too: the reference's key set holds it.
// Per item: one butterfly per touched slot, ONE 64-bit atomic add instruction (lane s: slot s, then total and rows) and one atomic OR.
#include "mkp_dev_chunks.hpp"
#include "mkp_dev_dmr_filter.hpp"
#include "mkp_launch.h"

namespace {

__global__ __launch_bounds__(256) void mkp_dmr_reduce(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ info,
    const uint32_t* __restrict__ code, const uint32_t* __restrict__ n_valid, const uint32_t* __restrict__ n_mod, const uint32_t* __restrict__ n_can,
    const MkpStatsRegion* __restrict__ regions, uint32_t n_regions, const uint32_t* __restrict__ row_lo, const uint32_t* __restrict__ row_hi,
    const unsigned long long* __restrict__ off, const unsigned long long* __restrict__ total_p, const uint8_t* __restrict__ ref, uint32_t ref_off,
    uint32_t ref_len, const MkpDmrParams P, unsigned long long* __restrict__ out, uint32_t* __restrict__ seen, uint32_t* codes, uint32_t* err) {
  const int lane = lane_id();
  const unsigned long long n_waves = (unsigned long long)gridDim.x * (blockDim.x >> 6), total = *total_p;
  uint32_t tab = load_codes(codes, lane);   // the code table as this wave last saw it
  for (unsigned long long w = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < total; w += n_waves) {
    const uint32_t a = item_region(off, n_regions, w);
    const MkpStatsRegion g = regions[a];
    const uint32_t lo = row_lo[a], hi = row_hi[a], first = lo + (uint32_t)(w - off[a]) * kChunk, last = min(first + kChunk, hi);
    unsigned long long am[kSlots], tot = 0, n_part = 0;
#pragma unroll
    for (int s = 0; s < kSlots; s++) am[s] = 0;
    uint32_t touched = 0; bool bad = false;
    for (uint32_t base = first; base < last; base += 64u) {
      const uint32_t i = base + (uint32_t)lane;
      uint32_t p = 0, bidx = 4u, listed = 2u, c = 0, nv = 0, nm = 0, nc = 0;
      // the rows in front of and behind this lane's row, loaded with it (their cache lines are the row's own or the next ones): most groups
      // are two rows, and neither the look backwards nor the first step of the walk then waits for a second round of loads
      uint32_t prev_p = 0, prev_s = 0, prev_c = 0, prev_nv = 0, next_p = 0, next_s = 0, next_c = 0, next_nv = 0, next_nm = 0, next_nc = 0;
      bool has_prev = false, has_next = false;
      bool walking = false;   // this lane's row is the first of its group
      if (i < last) {
        p = pos[i]; c = code[i]; nv = n_valid[i]; nm = n_mod[i]; nc = n_can[i];
        const uint32_t sidx = info[i] & 3u;
        has_prev = i > lo; has_next = i + 1u < hi;
        if (has_prev) { prev_p = pos[i - 1]; prev_s = info[i - 1] & 3u; prev_c = code[i - 1]; prev_nv = n_valid[i - 1]; }
        if (has_next) { next_p = pos[i + 1]; next_s = info[i + 1] & 3u; next_c = code[i + 1]; next_nv = n_valid[i + 1]; next_nm = n_mod[i + 1];
          next_nc = n_can[i + 1]; }
        const uint32_t at = p - ref_off;
        if (p >= ref_off && at < ref_len) bidx = base_index(ref[at], P.mask != 0u);
        listed = listed_strand(P, bidx, g.rule);
        walking = takes_part(P, bidx, listed, sidx, c, nv);
        if (walking && has_prev && prev_p == p) {
          if (takes_part(P, bidx, listed, prev_s, prev_c, prev_nv)) walking = false;
          for (uint32_t j = i - 1u; walking && j > lo && pos[j - 1] == p; j--)
            if (takes_part(P, bidx, listed, info[j - 1] & 3u, code[j - 1], n_valid[j - 1])) walking = false;
        }
      }
      // the group walk, one row a step: (c, nv, nm, nc) = the row lane's walk stands on, part = it takes part
      const uint32_t g_nv = nv, g_nc = nc;
      unsigned long long g_mod = 0;
      const bool head = walking;
      bool part = walking;
      uint32_t j = i;
      while (__ballot(walking)) {
        const int slot = resolve_slot(tab, codes, err, walking && part, c, true, lane);
        if (walking && part) {
          if (slot >= 0) touched |= 1u << slot;
#pragma unroll
          for (int s = 0; s < kSlots; s++) am[s] += slot == s ? nm : 0u;
          g_mod += nm; n_part++;
          if (nv != g_nv || nc != g_nc) bad = true;
        }
        if (walking) {
          j++;
          uint32_t sidx = 0;
          if (j == i + 1u) { walking = has_next && next_p == p; c = next_c; nv = next_nv; nm = next_nm; nc = next_nc; sidx = next_s; }
          else if (j < hi && pos[j] == p) { c = code[j]; nv = n_valid[j]; nm = n_mod[j]; nc = n_can[j]; sidx = info[j] & 3u; }
          else walking = false;
          if (walking) part = takes_part(P, bidx, listed, sidx, c, nv);
        }
      }
      if (head) { if ((unsigned long long)g_nc + g_mod != (unsigned long long)g_nv) bad = true; tot += g_nv; }
    }
    touched = wave_or(touched);
    const bool any_bad = __ballot(bad) != 0ull;
    if (!touched && !any_bad) continue;
    unsigned long long mine = 0;
#pragma unroll
    for (int s = 0; s < kSlots; s++) if ((touched >> s) & 1u) {   // (wave-uniform)
      const unsigned long long sm = wave_sum_u64(am[s]);
      if (lane == s) mine = sm;
    }
    const unsigned long long st = wave_sum_u64(tot), sp = wave_sum_u64(n_part);
    if (lane == MKP_DMR_CELL_TOTAL) mine = st;
    if (lane == MKP_DMR_CELL_ROWS) mine = sp;
    if (lane < MKP_DMR_CELLS && mine) atomicAdd(&out[(size_t)g.out * MKP_DMR_CELLS + (uint32_t)lane], mine);
    if (lane == 0) atomicOr(&seen[g.out], touched | (any_bad ? MKP_DMR_SEEN_BAD : 0u));
  }
}

}  // namespace

// host-side launcher (declared in mkp_launch.h).  ev (may be NULL): three events recorded in front of the bounds kernel, in front of the reduce
// kernel and behind it
extern "C" hipError_t mkp_launch_dmr(hipStream_t st, const uint32_t* pos, const uint32_t* info, const uint32_t* code, const uint32_t* n_valid,
    const uint32_t* n_mod, const uint32_t* n_can, uint32_t n_rows, const MkpStatsRegion* regions, uint32_t n_regions, uint32_t* row_lo,
    uint32_t* row_hi, uint32_t* n_chunks, unsigned long long* off, unsigned long long* total, const uint8_t* ref, uint32_t ref_off, uint32_t ref_len,
    const MkpDmrParams* prm, unsigned long long* out, uint32_t* seen, uint32_t* codes, uint32_t* err, hipEvent_t* ev) {
  if (!n_rows || !n_regions) return hipSuccess;
  hipError_t e;
  if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return e;
  mkp_stats_bounds<<<(n_regions + 255u) / 256u, 256, 0, st>>>(pos, n_rows, regions, n_regions, row_lo, row_hi, n_chunks);
  mkp_stats_scan<<<1, 1024, 0, st>>>(n_chunks, n_regions, off, total);
  if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return e;
  const unsigned long long most = (unsigned long long)n_regions * ((n_rows + MKP_STATS_CHUNK - 1u) / MKP_STATS_CHUNK);
  const uint32_t blocks = (uint32_t)std::min<unsigned long long>((most + 3ull) / 4ull, 4096ull);
  mkp_dmr_reduce<<<blocks, 256, 0, st>>>(pos, info, code, n_valid, n_mod, n_can, regions, n_regions, row_lo, row_hi, off, total, ref, ref_off,
      ref_len, *prm, out, seen, codes, err);
  if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return e;
  return hipGetLastError();
}
