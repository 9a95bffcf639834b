// The work-item scheme the region reducers over resident bedMethyl rows share (mkp_stats.hip, mkp_dmr.hip): one thread per region finds its
// rows, one workgroup scans the regions' chunk counts, and the reduce kernel of each feature takes one wave per (region, 4096-row chunk)
// item on a fixed strided grid; the 64-bit butterfly sum its items end with.
#pragma once
#include "mkp_dev_codeslots.hpp"

namespace {

constexpr uint32_t kChunk = MKP_STATS_CHUNK;

__global__ __launch_bounds__(256) void mkp_stats_bounds(const uint32_t* __restrict__ pos, uint32_t n_rows, const MkpStatsRegion* __restrict__ regions,
    uint32_t n_regions, uint32_t* __restrict__ row_lo, uint32_t* __restrict__ row_hi, uint32_t* __restrict__ n_chunks) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_regions) return;
  const MkpStatsRegion g = regions[r];
  uint32_t lo, hi;
  row_range(pos, n_rows, g.start, g.end, &lo, &hi);
  row_lo[r] = lo; row_hi[r] = hi; n_chunks[r] = (hi - lo + kChunk - 1) / kChunk;
}

// off[r] = chunks of the regions before r, off[n_regions] = *total = all of them (64-bit: a million regions of a whole chromosome each)
__global__ __launch_bounds__(1024) void mkp_stats_scan(const uint32_t* __restrict__ n_chunks, uint32_t n_regions, unsigned long long* __restrict__ off,
    unsigned long long* __restrict__ total) {
  __shared__ unsigned long long part[1024];
  const uint32_t t = threadIdx.x, per = (n_regions + 1023u) / 1024u;
  const uint32_t r0 = min(t * per, n_regions), r1 = min(r0 + per, n_regions);
  unsigned long long mine = 0;
  for (uint32_t r = r0; r < r1; r++) mine += n_chunks[r];
  part[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const unsigned long long add = t >= d ? part[t - d] : 0ull;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  unsigned long long run = part[t] - mine;
  for (uint32_t r = r0; r < r1; r++) { off[r] = run; run += n_chunks[r]; }
  if (t == 1023u) { off[n_regions] = part[t]; *total = part[t]; }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// the region of item w: the last one whose offset is <= w (regions without rows share their successor's offset and are never found)
__device__ __forceinline__ uint32_t item_region(const unsigned long long* __restrict__ off, uint32_t n_regions, unsigned long long w) {
  uint32_t a = 0, b = n_regions;   // off[a] <= w < off[b]
  while (b - a > 1) { const uint32_t mid = a + ((b - a) >> 1); if (off[mid] <= w) a = mid; else b = mid; }
  return a;
}

}  // namespace
