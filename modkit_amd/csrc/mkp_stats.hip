// Region statistics (`modkit stats`, src/stats/mod.rs:53-101) over bedMethyl rows that are already in HBM: per region and mod code,
// n_mod = sum of N_mod and n_valid = sum of N_valid_cov over the rows whose position lies in [start, end), whose strand overlaps the
// region's rule (StrandRule::overlaps, src/util.rs:310-318) and whose N_valid_cov reaches --min-coverage.
//
// Input: the SoA row columns of one piece of one contig, ascending in `pos`, and the regions of that contig (any order; they may overlap,
// nest and repeat, so this is not one segmented scan).  Three launches on the caller's stream, no host round trip between them:
//   mkp_stats_bounds   one thread per region: lower_bound(start) / lower_bound(end) in `pos` and the number of 4096-row chunks in between
//   mkp_stats_scan     one workgroup: exclusive prefix sum of the chunk counts (64-bit) and their total
//   mkp_stats_reduce   one WAVE per (region, chunk) work item, four to a workgroup, a fixed grid striding over the items: 64 rounds of
//                      64 coalesced rows (info, code, n_valid, n_mod: 16 of a row's 44 bytes), per-lane 64-bit sums per code slot, one
//                      butterfly per touched slot and ONE 64-bit atomic add instruction per item: lane 2 s adds n_mod, lane 2 s + 1
//                      n_valid of slot s — 256 contiguous bytes of the region's line of the run-long table.
// A whole-chromosome region is 660 items spread over the grid; thirty thousand 50-row regions are 7 500 workgroups' worth of waves.
// The table out[region][slot] lives for the whole run: pieces (shards) add into it, so a region that straddles seams gets every row once.
// Code slots: at most MKP_STATS_MAX_CODES per run.  With a fixed list the host uploads the table and other codes are not counted; without
// one, the first counted row of a code claims a free entry with a compare-and-swap (order does not matter, the host sorts): resolve_slot
// of mkp_dev_codeslots.hpp, which also holds the two searches of the bounds kernel; both are shared with mkp_localize.hip.  The bounds and
// scan kernels and the butterfly live in mkp_dev_chunks.hpp: mkp_dmr.hip runs the same scheme.
#include "mkp_dev_chunks.hpp"
#include "mkp_launch.h"

namespace {

__global__ __launch_bounds__(256) void mkp_stats_reduce(const uint32_t* __restrict__ info, const uint32_t* __restrict__ code,
    const uint32_t* __restrict__ n_valid, const uint32_t* __restrict__ n_mod, const MkpStatsRegion* __restrict__ regions, uint32_t n_regions,
    const uint32_t* __restrict__ row_lo, const uint32_t* __restrict__ row_hi, const unsigned long long* __restrict__ off,
    const unsigned long long* __restrict__ total_p, unsigned long long* __restrict__ out, uint32_t* __restrict__ seen, uint32_t* codes,
    uint32_t* err, unsigned long long min_cov, uint32_t fixed_codes) {
  const int lane = lane_id();
  const unsigned long long n_waves = (unsigned long long)gridDim.x * (blockDim.x >> 6), total = *total_p;
  uint32_t tab = load_codes(codes, lane);   // the code table as this wave last saw it
  for (unsigned long long w = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < total; w += n_waves) {
    const uint32_t a = item_region(off, n_regions, w);
    const MkpStatsRegion g = regions[a];
    const uint32_t first = row_lo[a] + (uint32_t)(w - off[a]) * kChunk, last = min(first + kChunk, row_hi[a]);
    unsigned long long am[kSlots], av[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; s++) { am[s] = 0; av[s] = 0; }
    uint32_t touched = 0;
    for (uint32_t base = first; base < last; base += 64u) {
      const uint32_t i = base + (uint32_t)lane;
      bool pass = false; uint32_t c = 0, nv = 0, nm = 0;
      if (i < last) {
        const uint32_t sidx = info[i] & 3u;   // 0 '+', 1 '-', 2 '.'
        c = code[i]; nv = n_valid[i]; nm = n_mod[i];
        pass = (g.rule == 3u || sidx == 2u || sidx + 1u == g.rule) && (unsigned long long)nv >= min_cov;
      }
      const int slot = resolve_slot(tab, codes, err, pass, c, !fixed_codes, lane);
      if (slot >= 0) touched |= 1u << slot;
#pragma unroll
      for (int s = 0; s < kSlots; s++) { const bool m = slot == s; am[s] += m ? nm : 0u; av[s] += m ? nv : 0u; }
    }
    touched = wave_or(touched);
    if (!touched) continue;
    unsigned long long mine = 0;
#pragma unroll
    for (int s = 0; s < kSlots; s++) if ((touched >> s) & 1u) {   // (wave-uniform)
      const unsigned long long sm = wave_sum_u64(am[s]), sv = wave_sum_u64(av[s]);
      if (lane == 2 * s) mine = sm;
      if (lane == 2 * s + 1) mine = sv;
    }
    if (lane < 2 * kSlots && ((touched >> (lane >> 1)) & 1u)) atomicAdd(&out[(size_t)g.out * (2 * kSlots) + (uint32_t)lane], mine);
    if (lane == 0) atomicOr(&seen[g.out], touched);
  }
}

}  // namespace

// host-side launcher (declared in mkp_launch.h).  ev (may be NULL): three events recorded in front of the bounds kernel, in front of the reduce
// kernel and behind it
extern "C" hipError_t mkp_launch_region_stats(hipStream_t st, const uint32_t* pos, const uint32_t* info, const uint32_t* code, const uint32_t* n_valid,
    const uint32_t* n_mod, uint32_t n_rows, const MkpStatsRegion* regions, uint32_t n_regions, uint32_t* row_lo, uint32_t* row_hi, uint32_t* n_chunks,
    unsigned long long* off, unsigned long long* total, unsigned long long* out, uint32_t* seen, uint32_t* codes, uint32_t* err,
    unsigned long long min_cov, uint32_t fixed_codes, hipEvent_t* ev) {
  if (!n_rows || !n_regions) return hipSuccess;
  hipError_t e;
  if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return e;
  mkp_stats_bounds<<<(n_regions + 255u) / 256u, 256, 0, st>>>(pos, n_rows, regions, n_regions, row_lo, row_hi, n_chunks);
  mkp_stats_scan<<<1, 1024, 0, st>>>(n_chunks, n_regions, off, total);
  if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return e;
  // as many waves as there can be items, up to a grid that fills the chip a few times over
  const unsigned long long most = (unsigned long long)n_regions * ((n_rows + MKP_STATS_CHUNK - 1u) / MKP_STATS_CHUNK);
  const uint32_t blocks = (uint32_t)std::min<unsigned long long>((most + 3ull) / 4ull, 4096ull);
  mkp_stats_reduce<<<blocks, 256, 0, st>>>(info, code, n_valid, n_mod, regions, n_regions, row_lo, row_hi, off, total, out, seen, codes, err, min_cov,
      fixed_codes);
  if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return e;
  return hipGetLastError();
}
