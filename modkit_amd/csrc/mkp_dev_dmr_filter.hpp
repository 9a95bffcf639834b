// Which bedMethyl rows take part in `modkit dmr` (genome_positions.rs:91-127, bedmethyl.rs:172-267), shared by the region form
// (mkp_dmr.hip) and the single-site form (mkp_dmr_sites.hip): the reference base under a row, the strand get_positions lists it on, and
// the row filter itself.
#pragma once
#include "mkp_dev_common.hpp"

namespace {

// index in "ACGT" of a reference byte, 4 = no base
__device__ __forceinline__ uint32_t base_index(uint32_t b, bool mask) {
  if (!mask && b >= 'a' && b <= 'z') b -= 32u;
  return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
}

// the strand get_positions lists a reference base on: 0 '+', 1 '-', 2 = not listed
__device__ __forceinline__ uint32_t listed_strand(const MkpDmrParams& P, uint32_t bidx, uint32_t rule) {
  if (bidx > 3u) return 2u;
  if (((P.pos_set >> bidx) & 1u) && (rule & 1u)) return 0u;
  if (((P.neg_set >> bidx) & 1u) && (rule & 2u)) return 1u;
  return 2u;
}

// a row at a position whose reference base is bidx, listed on strand `listed`
__device__ __forceinline__ bool takes_part(const MkpDmrParams& P, uint32_t bidx, uint32_t listed, uint32_t sidx, uint32_t c, uint32_t nv) {
  if (listed > 1u || (unsigned long long)nv < P.min_cov) return false;
  uint32_t cb = 4u;
  for (uint32_t k = 0; k < P.n_lookup; k++) if (P.code[k] == c) cb = P.base[k];
  if (cb > 3u) return false;
  const uint32_t cls = sidx == 1u ? 1u : 0u;   // get_stranded_position: '-' is negative, '+' and '.' positive
  return cls == listed && (cls ? 3u - cb : cb) == bidx;
}

}  // namespace
