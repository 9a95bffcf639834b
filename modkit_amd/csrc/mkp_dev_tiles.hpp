// What the two tile bodies of mkp_kernels.hip (dense_tiles_body, hemi_tiles_body) share: the workgroup prologue, the tile remap,
// the read ticket, the skip over CIGAR chunks in front of the tile and the walk over a read's events inside the tile (the
// difference arrays of the observed codes are in mkp_dev_rows.hpp: the stream kernels use them too).  One job each; the walks
// themselves differ and stay in the bodies.
#pragma once
#include "mkp_dev_rows.hpp"

// Workgroup prologue (callers put a barrier behind it): the run's parameters go to LDS, and so does the table
// SEQ byte -> NoCall row of the base a query index selects, rowlut[strand][query parity][byte]; 15 = not A/C/G/T.
// (BAM packs two bases per byte, high nibble first; on the '-' strand the tallied base is the complement.)
__device__ __forceinline__ void tile_prologue(const MkpRunParams* __restrict__ prmp, uint8_t* __restrict__ rowlut, uint32_t* __restrict__ prm_lds) {
  static_assert(PILEUP_THREADS == 1024, "the row table is filled one entry per thread");
  const uint32_t t = threadIdx.x, byte = t & 255u, par = (t >> 8) & 1u, st = (t >> 9) & 1u;   // t = index of [st][par][byte]
  const uint32_t nib = par ? (byte & 15u) : (byte >> 4);
  const unsigned long long LUT = st ? 0xfffffff0fff1f23fULL : 0xfffffff3fff2f10fULL;
  rowlut[t] = (uint8_t)((LUT >> (4u * nib)) & 15u);
  for (uint32_t kq = threadIdx.x; kq < sizeof(MkpRunParams) / 4; kq += PILEUP_THREADS) prm_lds[kq] = reinterpret_cast<const uint32_t*>(prmp)[kq];
}

// XCD-aware mapping: consecutive workgroups land on different XCDs (b % 8); give each XCD a contiguous run of tiles so the reads
// shared by neighbouring tiles stay in one L2.  One workgroup per tile; the dispatcher hands tiles to CUs as workgroups retire.
__device__ __forceinline__ uint32_t xcd_tile_index(uint32_t n_tiles) {
  uint32_t tix = blockIdx.x;
  const uint32_t per = n_tiles / 8u;
  if (per && tix < per * 8u) tix = (tix & 7u) * per + (tix >> 3);
  return tix;
}

// Reads are handed out one at a time (LDS ticket) so waves finish the tile together whatever the reads' spans; the next read's
// header and decode summary are requested while the current read is processed (one global round trip less per read).
struct TileRead { uint32_t rid; MkpReadHdr h; MkpReadOut ro; };
__device__ __forceinline__ void draw_read(uint32_t* next_read, uint32_t rid_end, const MkpReadHdr* __restrict__ hdrs,
    const MkpReadOut* __restrict__ readout, TileRead& nx) {
  uint32_t ticket = 0;
  if (lane_id() == 0) ticket = atomicAdd(next_read, 1u);
  nx.rid = (uint32_t)__builtin_amdgcn_readfirstlane((int)ticket);
  const uint32_t r0 = min(nx.rid, rid_end - 1u);   // (tiles hold at least one candidate read)
  nx.h = hdrs[r0]; nx.ro = readout[r0];
}

// Where a read's CIGAR walk starts: the 64-op chunks that end before the tile are skipped through the host's per-chunk offsets.
struct CigarStart { uint32_t q_run; int32_t r_run; uint32_t c_first; };   // query / reference offset in front of op c_first
__device__ __forceinline__ CigarStart skip_chunks_before(const MkpReadHdr& h, const uint2* __restrict__ chunk_pfx, int32_t T0h) {
  CigarStart cs = {0u, h.ref_start, 0u};
  const uint32_t nch = (h.n_cigar + 63u) >> 6, lane = (uint32_t)lane_id();
  if (nch > 1 && T0h > h.ref_start) {
    const uint32_t rel = (uint32_t)(T0h - h.ref_start);
    for (uint32_t b0 = 0; b0 < nch; b0 += 64) {
      const uint32_t kidx = b0 + lane;
      const uint2 e = kidx < nch ? chunk_pfx[h.chunk_off + kidx] : make_uint2(0u, 0xffffffffu);
      const uint32_t cnt = (uint32_t)__popcll(__ballot(kidx < nch && e.y <= rel));   // offsets ascend: a prefix of the lanes
      if (cnt) {
        cs.q_run = (uint32_t)__builtin_amdgcn_readlane((int)e.x, (int)(cnt - 1u));
        cs.r_run = h.ref_start + (int32_t)__builtin_amdgcn_readlane((int)e.y, (int)(cnt - 1u));
        cs.c_first = 64u * (b0 + cnt - 1u);
      }
      if (cnt < 64u) break;
    }
  }
  return cs;
}

// The read's call events inside the tile (a position-sorted slice), 64 per step, one per lane: f(index, event).
// from_start: the read starts inside the tile, so no search for the first one.
template <class F>
__device__ __forceinline__ void for_tile_events(const MkpEvent* __restrict__ ev, uint32_t n_events, bool from_start, int32_t T0h, int32_t T1h, F f) {
  const uint32_t lo = from_start ? 0u : event_lower_bound(ev, n_events, T0h);
  for (uint32_t k = lo + (uint32_t)lane_id();; k += 64) {
    bool in = k < n_events;
    MkpEvent e; e.pos = 0; e.info = 0;
    if (in) { e = ev[k]; in = (int32_t)e.pos < T1h; }
    if (in) f(k, e);
    if (!__any(in)) break;
  }
}
