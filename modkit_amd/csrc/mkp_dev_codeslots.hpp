// What the reducers over resident bedMethyl rows (mkp_stats.hip, mkp_localize.hip) share on the device: the rows of a [from, to) interval of
// an ascending `pos` column, and the run-long table of at most MKP_STATS_MAX_CODES code slots — a wave's copy of it, the look-up of a row's
// code, and the claim of a free slot by the first counted row of a code.
#pragma once
#include "mkp_dev_common.hpp"

namespace {

constexpr int kSlots = MKP_STATS_MAX_CODES;

__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* __restrict__ a, uint32_t n, uint32_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}

// the rows [lo, hi) whose position lies in [from, to); an empty interval has none
__device__ __forceinline__ void row_range(const uint32_t* __restrict__ pos, uint32_t n_rows, uint32_t from, uint32_t to, uint32_t* lo, uint32_t* hi) {
  uint32_t a = 0, b = 0;
  if (to > from) { a = lower_bound_u32(pos, n_rows, from); b = lower_bound_u32(pos, n_rows, to); }
  *lo = a; *hi = b;
}

// the code table as this wave sees it now: entry s in lane s
__device__ __forceinline__ uint32_t load_codes(const uint32_t* codes, int lane) {
  return lane < kSlots ? __hip_atomic_load(&codes[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
}

// the slot whose code is c in the wave's copy of the table (entry s in lane s), or -1
__device__ __forceinline__ int find_slot(uint32_t tab, uint32_t c) {
  int slot = -1;
#pragma unroll
  for (int s = 0; s < kSlots; s++) { const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)tab, s); if (e == c) slot = s; }
  return slot;
}

// The slot of this lane's row (code c, counted when `pass`), or -1 for a lane without a counted row or a code that has no slot.  `tab` is
// the wave's copy of the table and is refreshed when a code is new to it.  With `may_claim` a code without a slot takes a free one with a
// compare-and-swap (order does not matter, the host sorts); a seventeenth code sets MKP_STATS_ERR_CODES in *err.
// EVERY lane of the wave must reach this call (the ballots and shuffles are wave-wide): call it outside any lane-dependent branch and from
// loops whose trip count is wave-uniform, idle lanes with pass = false.
__device__ __forceinline__ int resolve_slot(uint32_t& tab, uint32_t* codes, uint32_t* err, bool pass, uint32_t c, bool may_claim, int lane) {
  int slot = find_slot(tab, c);
  if (!pass) slot = -1;   // (c == 0 of an idle lane matches the free entries)
  if (may_claim && __ballot(pass && slot < 0)) {
    // a code this wave has not met: look again (another wave has usually claimed it by now), then ONE lane per distinct code claims —
    // every lane of every wave of a fresh launch meets an empty table, and their compare-and-swaps would all queue on one cache line
    tab = load_codes(codes, lane);
    slot = find_slot(tab, c);
    if (!pass) slot = -1;
    bool missing = pass && slot < 0;
    unsigned long long miss = __ballot(missing);
    while (miss) {
      const int leader = __ffsll((long long)miss) - 1;
      const uint32_t c0 = (uint32_t)__shfl((int)c, leader, 64);
      int s0 = -1;
      if (lane == leader) {
        for (int s = 0; s < kSlots && s0 < 0; s++) { const uint32_t old = atomicCAS(&codes[s], 0u, c0); if (old == 0u || old == c0) s0 = s; }
        if (s0 < 0) atomicOr(err, MKP_STATS_ERR_CODES);
      }
      s0 = __shfl(s0, leader, 64);
      if (missing && c == c0) { slot = s0; missing = false; }
      miss = __ballot(missing);
    }
    tab = load_codes(codes, lane);
  }
  return slot;
}

}  // namespace
