// Device helpers the two single-site dmr files share (mkp_dmr_sites.hip, mkp_dmr_reps.hip): the workgroup rank of a flag, the batch a position
// lies in, and the per-code sums of a site's rows.
#pragma once
#include "mkp_dev_codeslots.hpp"
#include "mkp_dmr_site_math.hpp"

namespace {

// the number of set flags among the workgroup's lanes in front of this one, and (in *total) among all of them; sh: 2 * 4 words of LDS
__device__ __forceinline__ uint32_t block_rank(bool f, uint32_t* sh, uint32_t* total) {
  const unsigned long long m = __ballot(f);
  const uint32_t wave = threadIdx.x >> 6;
  if (lane_id() == 0) sh[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < (blockDim.x >> 6); w++) { const uint32_t v = sh[w]; if (w < wave) before += v; all += v; }
  __syncthreads();
  *total = all;
  return before + (uint32_t)__popcll(m & lanemask_lt());
}

// the entry of the contig's batch table a position lies in (the first entry starts at 0)
__device__ __forceinline__ uint32_t batch_entry(const MkpDmrSitesBatch* __restrict__ batches, uint32_t n_entries, uint32_t p) {
  uint32_t lo = 0, hi = n_entries;   // the last entry with start <= p
  while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (batches[mid].start <= p) lo = mid; else hi = mid; }
  return lo;
}

// the participating rows of site `s` of a sample summed per code column: cnt[col] += N_mod, has |= 1 << col.  col_of_slot: 4 bits a slot
__device__ __forceinline__ void sum_group(const MkpDmrSitesSample& S, uint32_t s, unsigned long long col_of_slot, uint32_t (&cnt)[MKP_DMR_SITE_MAX_CODES],
    uint32_t* has) {
  const uint32_t p = S.s_pos[s];
  for (uint32_t j = S.s_first[s]; j < S.n_rows && S.pos[j] == p; j++) {
    const uint32_t f = S.rowflag[j];
    if (!(f & MKP_DMRS_ROW_PART)) continue;
    const uint32_t col = (uint32_t)(col_of_slot >> (4u * (f & MKP_DMRS_ROW_SLOT))) & 15u, nm = S.n_mod[j];
    *has |= 1u << col;
#pragma unroll
    for (uint32_t k = 0; k < MKP_DMR_SITE_MAX_CODES; k++) cnt[k] += col == k ? nm : 0u;
  }
}

}  // namespace
