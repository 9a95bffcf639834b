// gfx950 (CDNA4, wave64) kernels of the modkit-pileup hot path, part 1: the event pipeline.  Integer / byte work bound by
// instruction issue, LDS atomics and HBM — no MFMA.  (Part 2, mkp_slots.hip, is the slot pipeline focus runs take; it reuses the
// decode kernels below for the read classes its fused decoder does not cover.)  One device pass here, in order:
//
//   decode, one wave per read, one kernel per read class (host-built id lists, longest reads first):
//     mkp_decode_sparse1/2   one explicit-mode ('?') group, one shared delta list: 4096-base steps that only count (nibble flags,
//                            byte-packed popcounts, DPP scan); the listed ranks are located per call (lane search + SWAR select)
//     mkp_decode_fast1/2     one group, any mode / differing delta lists: 1024-base steps, ordinal bitmap in LDS + 4-bit deposit
//     mkp_decode_reads       everything else (<= 8 tags, `N` tags, duplex, repeated codes): combine_positions_to_probs per group
//     mkp_merge_duplex       duplex reads decoded one group per wave: interleave the two position-sorted event lists
//   The three decoders differ in how they locate calls (their producers: drivers over named stages, on shared steps — rank_batch,
//   window_take, mark_window, deposit_marks, stored_base_total); the per-call work (ML -> f32 BaseModProbs, classify_rule: edge filter,
//   ReDistribute collapse, MultipleThresholdModCaller::call; CIGAR mapping, one packed 8-byte event per mapped call), the read prologue and
//   epilogue are the shared helpers in front of them.  FAST and SPARSE run it in one consumer, consume_batch, on full batches of 64 calls.
//   mkp_sample_* = the same walks emitting argmax probabilities / summary classes (threshold estimate, sample-probs, summary).
//
//   mkp_pileup_tiles[_keyed][_wide]   runs without focus positions: accumulate + emit, one 1024-thread workgroup per tile, two per CU;
//                            LDS holds the tile's 16-bit-packed (or _wide: u32) strand tallies; waves draw the tile's reads from an
//                            LDS ticket (observed-code difference arrays, the read's event slice, the depth walk over its CIGAR);
//                            rows are produced straight from LDS (mkp_dev_rows.hpp)
//   mkp_pileup_tiles_hemi    pileup-hemi: the same frame over the '+' motif positions only, duplex pattern counters
//   mkp_hemi_failed_reads    pileup-hemi: the one NoCall per interval a record with failing tags leaves
//   mkp_scan_tiles, mkp_gather_rows   order the tiles' row runs (exclusive scan of the counts + coalesced copy).
//   mkp_sample_accumulate / _hist1, mkp_summary_accumulate   summaries of the threshold sample (two-level histograms), summary counts.
//
// Semantics follow /root/reference/src (cited inline); arithmetic that must be bit-exact is f32
// with contraction off (-ffp-contract=off) and IEEE division.
#include "mkp_dev_common.hpp"
#include "mkp_dev_rows.hpp"
#include "mkp_dev_tiles.hpp"
#include "mkp_launch.h"

// ----------------------------------------------------------------------------------------------
// What the three wave-per-read decoders share.  They differ in how they locate a read's calls (the producers); the read
// prologue and epilogue, the per-call rules of the reference and the event append are written once, here.
__device__ __forceinline__ uint32_t rfl_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float rfl_f(float v) { return __uint_as_float(rfl_u(__float_as_uint(v))); }

// Read prologue: the wave's read and its header; the read's layout (1216 B) goes to the wave's LDS slice once, every table
// lookup afterwards is an LDS read.  False = nothing to decode: no read for this wave, or a bad / tag-less read, whose empty
// summary is written here.  Wave-uniform values are made provably uniform (readfirstlane) so they live in SGPRs and load
// through the scalar cache.  id_mask strips the flag bits a read list may carry in its ids (rid_raw keeps them).
__device__ __forceinline__ bool read_prologue(const MkpReadHdr* __restrict__ hdrs, uint32_t n_reads, const uint32_t* __restrict__ read_ids,
    const MkpLayout* __restrict__ layouts, MkpReadOut* __restrict__ readout, uint32_t* __restrict__ lds_layouts, uint32_t id_mask,
    uint32_t& wib, uint32_t& rid_raw, MkpReadHdr& h, uint32_t*& lds_lay) {
  const int lane = lane_id();
  wib = rfl_u(threadIdx.x >> 6);
  const uint32_t widx = rfl_u(blockIdx.x * (blockDim.x >> 6)) + wib;
  if (widx >= n_reads) return false;
  rid_raw = rfl_u(read_ids[widx]);
  const uint32_t rid = rid_raw & id_mask;
  h = hdrs[rid];
  if ((h.flags & MKP_RF_BAD) || h.n_tags == 0) {
    MkpReadOut out; out.n_events = 0; out.ok = 0; out.obs[0] = 0; out.obs[1] = 0;
    if (lane == 0) readout[rid] = out;
    return false;
  }
  lds_lay = lds_layouts + wib * MKP_LAYOUT_DWORDS;
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(&layouts[h.layout]);
  for (int i = lane; i < MKP_LAYOUT_DWORDS; i += 64) lds_lay[i] = src[i];
  __builtin_amdgcn_wave_barrier();
  return true;
}

// a group descriptor that is the same for the whole wave: every field in SGPRs
__device__ __forceinline__ GroupRegs load_group_uniform(const uint32_t* gp) {
  GroupRegs g = load_group(gp);
  g.misc = rfl_u(g.misc); g.slots = rfl_u(g.slots); g.cids = rfl_u(g.cids); g.member_tags = rfl_u(g.member_tags);
#pragma unroll
  for (int k = 0; k < MKP_KMAX; k++) at(g.thr, k) = rfl_f(at(g.thr, k));
  g.thr_can = rfl_f(g.thr_can);
  return g;
}

// Per-tag constants of a single-group decoder, tags tb .. tb+n_tags of the layout, all on base b0: number of codes, the tag's
// map ([0:3] member index, [4+4i : 8+4i) local code of the tag's i-th code) and the set of its local codes.  Wave-uniform.
template <int NT>
__device__ __forceinline__ void tag_setup(const MkpLayout* lay, int tb, int n_tags, int b0, uint32_t (&t_nc)[NT], uint32_t (&tmu)[NT],
    uint32_t (&codes_t)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; t++) {
    t_nc[t] = 0; tmu[t] = 0; codes_t[t] = 0;
    if (t < n_tags) {
      t_nc[t] = rfl_u(lay->tags[tb + t].n_codes);
      tmu[t] = rfl_u(lay->tagmap[tb + t][b0]);
      for (uint32_t i = 0; i < t_nc[t]; i++) codes_t[t] |= 1u << ((tmu[t] >> (4 + 4 * i)) & 15u);
    }
  }
}

__device__ __forceinline__ bool read_trimmable(const MkpRunParams& prm, uint32_t L) {   // read_can_be_trimmed (mod_bam.rs:1668-1671)
  return !prm.edge_filter || !(L <= prm.edge_start || L <= prm.edge_end);
}
__device__ __forceinline__ bool collapse_on(const MkpRunParams& prm) { return prm.numeric_mode == 2; }
// --edge-filter on the forward (as-sequenced) position f of a call
__device__ __forceinline__ bool edge_keep(const MkpRunParams& prm, uint32_t f, uint32_t L) {
  return !prm.edge_filter || (prm.edge_inverted ? (f < prm.edge_start || f >= L - prm.edge_end) : (f >= prm.edge_start && f < L - prm.edge_end));
}
// SeqPosBaseModProbs::filter_positions (read_ids_to_base_mod_probs.rs:966-1070); strand = the strand the call is tallied on
__device__ __forceinline__ bool sample_keep(const MkpRunParams& prm, const uint8_t* __restrict__ bedmask, bool mapped, int32_t rpos, uint32_t strand) {
  bool keep = !prm.only_mapped || mapped;
  if (prm.has_focus) keep = keep && mapped && rpos >= prm.win_start && rpos < prm.win_end && ((bedmask[rpos - prm.win_start] >> strand) & 1u);
  return keep;
}
// Which hit pattern of its group a call falls under: the members whose tags list it (SH) or, listed by none, the group's
// implicit-mode members, every occurrence of whose base is a call (implicit fill, mod_bam.rs:1265-1292).  False = no call here.
__device__ __forceinline__ bool call_pattern(uint32_t SH, uint32_t impl, bool& err, int& pat, uint32_t& members) {
  if (SH) { if (impl & ~SH) err = true; pat = (int)SH; members = SH; return true; }   // ExplicitConflictInferred
  pat = MKP_PAT_INFERRED; members = impl;
  return impl != 0u;
}
// counter id of a call: cls as call_group returns it
__device__ __forceinline__ uint32_t call_cid(const GroupRegs& g, int cls) {
  return cls == 0 ? (uint32_t)MKP_C_FAIL : cls == 1 ? MKP_G_CIDCAN(g.misc) : ((g.cids >> (8 * (cls - 2))) & 0xffu);
}
// the tags (bit per tag index) behind a set of group members
__device__ __forceinline__ uint32_t member_tagbits(uint32_t members, uint32_t member_tags) {
  uint32_t tagbits = 0;
#pragma unroll
  for (int mi = 0; mi < MKP_MAX_MEMBERS; mi++) if (members & (1u << mi)) tagbits |= 1u << ((member_tags >> (4 * mi)) & 15u);
  return tagbits;
}
// InvalidImplicitMode: a group all of whose contributing tags have no mode character (read_cache.rs:122-137)
__device__ __forceinline__ bool lacks_mode(uint32_t tagbits, uint32_t default_mask) { return tagbits && (tagbits & ~default_mask) == 0; }
// a delta list must not run past the last occurrence of its base / the end of the read: every entry must have been consumed
// by the join (mod_bam.rs:705-727, 750-756).  Reverse reads consume their list from its end.
__device__ __forceinline__ bool list_left_over(bool rev, uint32_t cur, uint32_t n) { return rev ? (cur != 0u) : (cur != n); }

#define DECODE_PARAMS(PRM) const MkpReadHdr* __restrict__ hdrs, uint32_t n_reads, const uint32_t* __restrict__ cigar, const uint8_t* __restrict__ seqs, \
                    const MkpTagRef* __restrict__ tagref, const uint32_t* __restrict__ ranks, const uint8_t* __restrict__ ml, \
                    const MkpLayout* __restrict__ layouts, PRM prm, MkpEvent* __restrict__ events, MkpReadOut* __restrict__ readout, \
                    uint32_t* __restrict__ dev_err, const uint8_t* __restrict__ bedmask, float* __restrict__ sample_vals, const uint32_t* __restrict__ read_ids
#define DECODE_PASS hdrs, n_reads, cigar, seqs, tagref, ranks, ml, layouts, prm, events, readout, dev_err, bedmask, sample_vals, read_ids

// ---- producer steps.  A tag's calls are a sorted list of ranks (forward-order ordinals of the tag's base, or positions for `N` tags);
// the read is walked in steps of stored bases, and every step takes the ranks of its window from the list's cursor.
// The 64 entries of a rank list at its cursor, one per lane: forward reads go up from it, reverse reads (whose walk meets the list's end first) down.
struct RankBatch { uint32_t e; bool valid; };
__device__ __forceinline__ RankBatch rank_batch(const uint32_t* __restrict__ ranks, uint32_t off, uint32_t n, uint32_t cur, bool rev) {
  const uint32_t i = (rev ? cur - 64u : cur) + (uint32_t)lane_id();
  RankBatch b; b.valid = rev ? ((int32_t)i >= 0 && i < cur) : (i < n);
  b.e = rev ? 0u : 0xffffffffu;
  if (b.valid) b.e = ranks[off + i];
  return b;
}
// The batch's entries inside the step's rank window [wlo, whi) are taken: hit, the lanes holding one, their number, the cursor moved
// past them (a forward entry >= whi of the last step is past the last occurrence: never consumed, an error at the end).  SUFFIX: the
// caller knows every entry to lie below whi (reverse reads of the SPARSE decoder) — the hits are a suffix of the batch.
struct RankTake { bool hit; unsigned long long lanes; uint32_t nh; };
template <bool SUFFIX = false>
__device__ __forceinline__ RankTake window_take(const RankBatch& b, uint32_t wlo, uint32_t whi, bool rev, uint32_t& cur) {
  RankTake t; t.hit = b.valid && (rev ? (b.e >= wlo && (SUFFIX || b.e < whi)) : (b.e < whi));
  t.lanes = __ballot(t.hit); t.nh = (uint32_t)__popcll(t.lanes);
  cur = rev ? cur - t.nh : cur + t.nh;
  return t;
}
// step-relative stored ordinal of a taken rank e: tot = the read's total of that base, first = the ordinals in front of the step
__device__ __forceinline__ uint32_t step_ordinal(uint32_t e, bool rev, uint32_t tot, uint32_t first) { return (rev ? (tot - 1u - e) : e) - first; }
// Every rank of the window [wlo, whi) marked as a bit of the step's ordinal bitmap in LDS (cleared by the caller; a wave_lds_sync
// before it is read).  `b` = the batch at the cursor, which the caller may have requested early.
__device__ __forceinline__ void mark_window(const uint32_t* __restrict__ ranks, uint32_t off, uint32_t n, uint32_t& cur, bool rev, RankBatch b,
    uint32_t wlo, uint32_t whi, uint32_t tot, uint32_t first, uint32_t* __restrict__ ordb) {
  for (;;) {
    const RankTake t = window_take(b, wlo, whi, rev, cur);
    if (t.nh == 0) break;
    const uint32_t ib = step_ordinal(b.e, rev, tot, first);
    if (t.hit) atomicOr(&ordb[ib >> 5], 1u << (ib & 31u));
    if (t.nh < 64) break;
    b = rank_batch(ranks, off, n, cur, rev);
  }
}
// Bits [ex, ex + popc(m)) of the ordinal bitmap deposited onto the set bits of the lane's W-base match mask m, four bases at a
// time (pdep4); ex = the occurrences in the lanes below.  The bitmap ends with the words the 64-bit window read may touch.
template <int W>
__device__ __forceinline__ uint32_t deposit_marks(const uint32_t* __restrict__ ordb, const uint8_t* __restrict__ pdep4, uint32_t m, uint32_t ex) {
  const uint32_t w0 = ordb[ex >> 5], w1 = ordb[(ex >> 5) + 1];
  const uint32_t f = __builtin_amdgcn_alignbit(w1, w0, ex & 31u) & ((1u << __popc(m)) - 1u);
  uint32_t bm = 0;
#pragma unroll
  for (int k = 0; k < W; k += 4)   // the mask's nibble at k takes the bits behind those of the nibbles below it
    bm |= (uint32_t)pdep4[(((m >> k) & 15u) << 4) | ((f >> __popc(m & ((1u << k) - 1u))) & 15u)] << k;
  return bm;
}
// The low nibble of a read's last byte is not a base when L is odd: the dword holding it and the mask that clears its flag
struct OddTail { uint32_t dw, clear; };
__device__ __forceinline__ OddTail odd_tail(uint32_t L) {
  OddTail o; o.dw = (L & 1u) ? ((L - 1u) >> 3) : 0xffffffffu; o.clear = ~(1u << (8u * (((L - 1u) >> 1) & 3u)));
  return o;
}
// Occurrences of stored base xs in the whole read, four loads in flight.  Reverse reads need it up front: forward rank =
// total - inclusive count in stored order.  The SEQ invariant the decoders' nibble flags rely on, stated once: both packers
// (mkp_pack.hpp, ingest_copy_record) zero-pad a read's SEQ to a dword and code 0 matches no base, so only the low nibble of an
// odd read's last byte needs clearing (odd_tail); dwords past the read are not loaded.
__device__ __forceinline__ uint32_t stored_base_total(const uint32_t* __restrict__ seqw, uint32_t nd, uint32_t L, int xs) {
  const uint32_t lane = (uint32_t)lane_id(), pat = 0x11111111u << xs;
  const OddTail odd = odd_tail(L);
  uint32_t acc = 0;
  for (uint32_t d0 = 0; d0 < nd; d0 += 256) {
    uint32_t xw[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { const uint32_t dd = d0 + 64u * j + lane; xw[j] = dd < nd ? seqw[dd] : 0u; }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t F = nibble_eq(xw[j], pat); if (d0 + 64u * j + lane == odd.dw) F &= odd.clear;
      acc += (uint32_t)__popc(F);
    }
  }
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(acc), 63);
}

// The read as its producer walks it: step after step of stored bases.
struct ReadWalk {
  const uint32_t* __restrict__ seqw; uint32_t L, nd; bool rev;
  uint32_t tot = 0;          // reverse reads: occurrences of the counted base in the whole read
  uint32_t cum = 0, d0 = 0;  // occurrences in front of the step, the step's first SEQ dword
};
// the rank lists of the decoder's tags, their ML arrays and the merge join's cursors (reverse reads start at the end)
template <int NT> struct TagLists { uint32_t off[NT], n[NT], ml[NT], cur[NT]; };
template <int NT>
__device__ __forceinline__ void tag_lists(const MkpTagRef* __restrict__ tagref, uint32_t first, int n_tags, bool rev, TagLists<NT>& T) {
#pragma unroll
  for (int t = 0; t < NT; t++) {
    T.off[t] = 0; T.n[t] = 0; T.ml[t] = 0; T.cur[t] = 0;
    if (t < n_tags) { const MkpTagRef tr = tagref[first + t]; T.off[t] = tr.rank_off; T.n[t] = tr.n; T.ml[t] = tr.ml_off; T.cur[t] = rev ? tr.n : 0u; }
  }
}

// What a read's calls add up to.  Per-lane while the read is walked; read_epilogue reduces it over the wave.
struct ReadAcc { bool err = false, any_surviving = false; uint32_t obs0 = 0, obs1 = 0, n_ev = 0; };

// Reference position through a 64-op CIGAR window held in registers, one op per lane, advanced as the walk moves along the read
// (aligned pairs: M/=/X only, util.rs:122-145).  Per op the inclusive query end and (reference start - query start): rpos = q + dl.
struct CigarWin { uint32_t c0 = 0, wq0 = 0, wq1 = 0; int32_t wr0; uint32_t w_op = 5u, w_qe = 0; int32_t w_dl = 0; uint32_t w_rtot = 0; bool loaded = false; };
// maps the query positions q of the lanes with `pending`; positions ascend from call to call, none lies before the window
__device__ __forceinline__ void cigar_map(CigarWin& w, const MkpReadHdr& h, const uint32_t* __restrict__ cigar, bool pending, uint32_t q,
    bool& mapped, int32_t& rpos) {
  const int lane = lane_id();
  for (;;) {
    if (!w.loaded || (__any(pending && q >= w.wq1) && !__any(pending && q < w.wq1))) {   // load / advance the window
      if (w.loaded) { w.c0 += 64; w.wq0 = w.wq1; w.wr0 += (int32_t)w.w_rtot; }
      if (w.c0 >= h.n_cigar) break;
      const uint32_t cw = (w.c0 + lane < h.n_cigar) ? cigar[h.cigar_off + w.c0 + lane] : 5u /*0H*/;
      w.w_op = cw & 15u; const uint32_t len = cw >> 4;
      const uint32_t qlen = op_consumes_query(w.w_op) ? len : 0u, rlen = op_consumes_ref(w.w_op) ? len : 0u;
      w.w_qe = wave_incl_scan(qlen); const uint32_t re = wave_incl_scan(rlen);
      w.w_dl = (w.wr0 + (int32_t)(re - rlen)) - (int32_t)(w.wq0 + w.w_qe - qlen);
      w.wq1 = w.wq0 + (uint32_t)__builtin_amdgcn_readlane((int)w.w_qe, 63); w.w_rtot = (uint32_t)__builtin_amdgcn_readlane((int)re, 63);
      w.loaded = true;
      continue;
    }
    const bool ready = pending && q < w.wq1;
    const int oi = find_op(w.w_qe, ready ? q - w.wq0 : 0u) & 63;
    const uint32_t my_op = __shfl(w.w_op, oi, 64);
    const int32_t my_dl = __shfl(w.w_dl, oi, 64);
    if (ready) { mapped = op_is_match(my_op); rpos = (int32_t)q + my_dl; pending = false; }
    if (!__any(pending)) break;
  }
}

// (CigarWin goes in and comes back by value: behind the reference mkp_decode_fast1 takes 67 VGPRs for 64 and loses its eighth wave)
template <bool SAMPLE>
__device__ __forceinline__ void map_window(CigarWin& w, const MkpReadHdr& h, const uint32_t* __restrict__ cigar, bool pending, uint32_t q,
    bool& mapped, int32_t& rpos) { CigarWin v = w; cigar_map(v, h, cigar, pending, q, mapped, rpos); w = v; }

// Call queue of the single-group decoders (N SoA columns of `stride` entries in LDS): move the (< 64) unconsumed entries to the front
template <int N> __device__ __forceinline__ void queue_to_front(uint32_t* __restrict__ q, uint32_t stride, uint32_t& qhead, uint32_t& qcount) {
  const uint32_t lane = (uint32_t)lane_id(), n_left = qcount - qhead;
  const bool mv = lane < n_left;
  uint32_t v[N];
#pragma unroll
  for (int c = 0; c < N; c++) v[c] = mv ? q[c * stride + qhead + lane] : 0u;
  wave_lds_sync();
#pragma unroll
  for (int c = 0; c < N; c++) if (mv) q[c * stride + lane] = v[c];
  qcount = n_left; qhead = 0;
}

// The ML bytes of one queued call per lane (up to MKP_KMAX per tag; get_base_mod_probs, mod_bam.rs:1242-1263: stride = #codes of
// the tag).  Requested first and converted after the CIGAR mapping, whose latency they overlap.  found[t]: tag t lists the
// lane's call, as its jx[t]-th.
template <int NT>
__device__ __forceinline__ void ml_prefetch(const uint8_t* __restrict__ ml, int n_tags, const uint32_t (&t_ml)[NT], const uint32_t (&t_nc)[NT],
    const bool (&found)[NT], const uint32_t (&jx)[NT], uint32_t (&mlq)[NT][MKP_KMAX]) {
#pragma unroll
  for (int t = 0; t < NT; t++) {
#pragma unroll
    for (int i = 0; i < MKP_KMAX; i++) mlq[t][i] = 0;
    if (t < n_tags) {
      const uint32_t nc = t_nc[t], base = found[t] ? (t_ml[t] + jx[t] * nc) : 0u;
#pragma unroll
      for (int i = 0; i < MKP_KMAX; i++) if ((uint32_t)i < nc) mlq[t][i] = ml[base + (found[t] ? (uint32_t)i : 0u)];
    }
  }
}
// ... and the call's probability map from them.  `check` (two or more tags list the call) asks for combine_checked's sum test
// over the local codes `setmask`, once on the final map (partial sums of positive terms cannot exceed it); true = it failed.
template <int NT>
__device__ __forceinline__ bool ml_to_probs(const uint32_t (&mlq)[NT][MKP_KMAX], int n_tags, const uint32_t (&t_nc)[NT], const uint32_t (&tmu)[NT],
    const bool (&found)[NT], uint32_t setmask, bool check, F4& pk) {
#pragma unroll
  for (int t = 0; t < NT; t++) {
    if (t >= n_tags) break;
#pragma unroll
    for (int i = 0; i < MKP_KMAX; i++) {
      if ((uint32_t)i >= t_nc[t]) break;
      const float p = ((float)mlq[t][i] + 0.5f) / 256.0f;   // quals_to_probs (mod_bam.rs:808-816)
      const uint32_t kk = (tmu[t] >> (4 + 4 * i)) & 15u;     // wave-uniform local code
      setk(pk, kk, found[t], p);
    }
  }
  if (NT == 1) return false;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MKP_KMAX; k++) if (setmask & (1u << k)) s = s + at(pk, k);
  return check && s > 1.01f;
}

// The per-call rule every decoder shares: one call at forward position f / reference position rpos on group g (base b, mod
// strand sg), pv = the group's entry for the call's hit pattern, pk = its probabilities.  Edge and trim gate, position filter
// of the sampling passes, then the pass's output.  True = the lane has an event: info (without bit 12, "first event of its
// position", which is the caller's), sample value in sv; ev_pos is touched only where the event's position is not rpos.
template <bool SAMPLE>
__device__ __forceinline__ bool classify_rule(const MkpRunParams& prm, const uint8_t* __restrict__ bedmask, const GroupRegs& g, uint32_t pv,
    int kcodes, int b, int sg, uint32_t aln, uint32_t L, bool trimmable, bool inferred, F4& pk, uint32_t f, bool mapped, int32_t rpos,
    ReadAcc& acc, uint32_t& ev_info, float& sv, int32_t& ev_pos) {
  if (!trimmable || !edge_keep(prm, f, L)) return false;
  const bool collapse = collapse_on(prm);
  const uint32_t tally = aln ^ (uint32_t)sg;  // read_cache.rs:181-188 / FeatureVector::add_feature
  uint32_t ob = 0;
  if (SAMPLE) {
    if (!sample_keep(prm, bedmask, mapped, rpos, tally)) return false;
    acc.any_surviving = true;
    if (prm.sample_mode < 2) { sv = argmax_group(g, pv, pk, collapse, kcodes); ev_info = MKP_G_TB(g.misc); return true; }
    // 2 `summary`: thresholded + argmax class; 3 `extract calls`: + forward position, mod strand, inferred, call_prob
    if (prm.sample_mode == 3 && ((pv >> 3) & 7u) == 0u) return false;   // the collapse left no code in the map: no profile row (iter_probs is empty)
    float am = 0.f;
    ev_info = summary_info(g, pv, pk, collapse, &ob, kcodes, &am); acc.obs0 |= ob;
    if (prm.sample_mode == 3) { ev_info |= ((uint32_t)sg << 2) | ((inferred ? 1u : 0u) << 3); sv = am; ev_pos = (int32_t)f; }
    return true;
  }
  acc.any_surviving = true;
  const int cls = call_group(g, pv, pk, collapse, &ob, kcodes);
  if (tally) acc.obs1 |= ob; else acc.obs0 |= ob;
  if (mapped) ev_info = call_cid(g, cls) | (tally << 8) | ((uint32_t)b << 9) | (aln << 11);
  return mapped;
}

// One call of a single-group decoder (group g, descriptor words at gp, on base b0 / mod strand sg0): SH = the members whose
// tags list it, impl = the group's implicit-mode members, pk = its probabilities, f / rpos = its forward and reference
// positions.  True = the lane has an event (info, position in rpos, sample value in sv).  INFER = false: the group has no
// implicit members (impl is not looked at), so SH is never empty.
template <bool SAMPLE, bool INFER>
__device__ __forceinline__ bool classify_call(const MkpRunParams& prm, const uint8_t* __restrict__ bedmask, const GroupRegs& g,
    const uint32_t* gp, int kcodes, int b0, int sg0, uint32_t aln, uint32_t L, bool trimmable, uint32_t SH, uint32_t impl, F4& pk,
    uint32_t f, bool mapped, int32_t& rpos, ReadAcc& acc, uint32_t& contribH, uint32_t& ev_info, float& sv) {
  int pat = (int)SH; uint32_t member_contrib = SH;
  if (INFER) call_pattern(SH, impl, acc.err, pat, member_contrib);   // the caller saw to SH | impl
  contribH |= member_contrib;
  int32_t pos = rpos;
  const bool has_ev = classify_rule<SAMPLE>(prm, bedmask, g, gp[12 + pat], kcodes, b0, sg0, aln, L, trimmable, INFER && pat == MKP_PAT_INFERRED,
                                            pk, f, mapped, rpos, acc, ev_info, sv, pos);
  rpos = pos;
  if (!SAMPLE && has_ev) ev_info |= 1u << 12;   // one event per position: it is the position's first
  return has_ev;
}

// Ballot-compacted, position-ordered append of one batch's events, up to N per lane (cnt of them, all at pos), to the read's
// event slice [ev_base, ev_base + ev_cap).  A slice too small is an error of the run (ERR_EVENT_CAP) and of the read.
template <bool SAMPLE, int N>
__device__ __forceinline__ void append_events(MkpEvent* __restrict__ events, float* __restrict__ sample_vals, uint32_t* __restrict__ dev_err,
    uint32_t ev_base, uint32_t ev_cap, uint32_t cnt, uint32_t pos, const uint32_t (&info)[N], const float (&sv)[N], ReadAcc& acc) {
  uint32_t step_total = 0, off = acc.n_ev;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const unsigned long long b = __ballot(cnt > (uint32_t)k);
    step_total += (uint32_t)__popcll(b); off += (uint32_t)__popcll(b & lanemask_lt());
  }
  if (!step_total) return;
  if (acc.n_ev + step_total > ev_cap) { acc.err = true; if (lane_id() == 0) atomicOr(dev_err, ERR_EVENT_CAP); }
  else {
#pragma unroll
    for (int k = 0; k < N; k++) if ((uint32_t)k < cnt) {
      MkpEvent ev; ev.pos = pos; ev.info = info[k]; events[ev_base + off + k] = ev;
      if (SAMPLE) sample_vals[ev_base + off + k] = sv[k];
    }
  }
  acc.n_ev += step_total;
}

// Read epilogue: the wave agrees on the outcome and lane 0 writes the read's summary.  ok = 1: decoded, with n_ev events;
// ok = 2 (idle_ok: a duplex half): this group added nothing (all of it edge-filtered) — the record still stands if the other group did.
__device__ __forceinline__ void read_epilogue(MkpReadOut* __restrict__ readout, uint32_t ro_idx, ReadAcc acc, bool idle_ok) {
  const bool err = __any(acc.err), any_surviving = __any(acc.any_surviving);
  MkpReadOut out; out.n_events = 0; out.ok = 0; out.obs[0] = 0; out.obs[1] = 0;
  if (!err && any_surviving) { out.ok = 1; out.n_events = acc.n_ev; out.obs[0] = wave_or(acc.obs0); out.obs[1] = wave_or(acc.obs1); }
  else if (!err && idle_ok) out.ok = 2;
  if (lane_id() == 0) readout[ro_idx] = out;
}

// ----------------------------------------------------------------------------------------------
// Decode, general layouts.  One wave per read.  The read is walked 512 bases at a time (one SEQ dword = 8 bases per lane):
//   general_base_slots     once per read: the distinct stored bases its tags count, and which of them carry implicit calls;
//   general_match_scan     per lane the match masks of those bases, popcounts, wave prefix sums (DeltaListConverter's cumulative
//                          counts, mod_bam.rs:667-684, 8 bases per instruction);
//   general_mark_deposit   per tag: the ranks of the chunk's window marked in an ordinal bitmap in LDS and deposited onto the lane's
//                          match mask (`N` tags: a position bitmap, read back as is) — an 8-bit "call here" mask per tag;
//   general_compact        the union of the masks (plus every occurrence of an implicit-mode base) as {lane, bit} slots in LDS;
//   then 64 positions per batch: general_position_probs (BaseModProbs in MM order, merge_tag per tag), cigar_map, general_classify
//   (classify_rule on the position's one or two groups), append_events.
// SAMPLE = threshold-sampling pass: emits argmax probabilities instead of call events.
// arr[j] for a wave-uniform j < N (N is tiny: a select chain, no scratch)
template <int N> __device__ __forceinline__ uint32_t selN(const uint32_t* a, uint32_t j) {
  uint32_t r = 0;   // OR of masked elements: a select chain over array elements is folded into an indexed (scratch) load
#pragma unroll
  for (int i = 0; i < N; i++) r |= (j == (uint32_t)i) ? a[i] : 0u;
  return r;
}
// The read's tags: lists, descriptors, and their base slots — the nb distinct stored bases (A,C,G,T = 0..3) some tag counts; implslots =
// the slots every occurrence of whose base is a call; per slot the read's total (reverse reads) and the occurrences in front of the chunk.
template <int NT, int NB> struct GeneralTags {
  TagLists<NT> T; MkpTagDesc desc[NT]; uint32_t tslot[NT];
  uint32_t sbase[NB], nb, implslots, tot[NB], cum[NB];
};
template <int NT, int NB>
__device__ __forceinline__ void general_base_slots(GeneralTags<NT, NB>& R, const MkpLayout* lay, const uint32_t* lds_lay, int n_tags, bool rev) {
  uint32_t nb = 0;
#pragma unroll
  for (int j = 0; j < NB; j++) { R.sbase[j] = 0; R.tot[j] = 0; R.cum[j] = 0; }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    R.tslot[t] = 0; R.desc[t] = lay->tags[t];
    if (t < n_tags && R.desc[t].fb != 4) {
      const uint32_t xb = (uint32_t)(rev ? 3 - R.desc[t].fb : R.desc[t].fb);
      uint32_t found = nb;
#pragma unroll
      for (int j = 0; j < NB; j++) if ((uint32_t)j < nb && R.sbase[j] == xb) found = (uint32_t)j;
      if (found == nb) {
#pragma unroll
        for (int j = 0; j < NB; j++) if ((uint32_t)j == nb) R.sbase[j] = xb;
        nb++;
      }
      R.tslot[t] = rfl_u(found);
    }
  }
  R.nb = rfl_u(nb);
  uint32_t implslots = 0;   // groups with implicit-mode members (mod_bam.rs:1265-1292)
#pragma unroll
  for (int j = 0; j < NB; j++) {
    R.sbase[j] = rfl_u(R.sbase[j]);
    const uint32_t b = rev ? 3u - R.sbase[j] : R.sbase[j];
    const uint32_t m0 = lds_lay[MKP_LAYOUT_GROUP_DW + b * 32], m1 = lds_lay[MKP_LAYOUT_GROUP_DW + (4 + b) * 32];
    if ((uint32_t)j < R.nb && (MKP_G_IMPL(m0) | MKP_G_IMPL(m1))) implslots |= 1u << j;
  }
  R.implslots = rfl_u(implslots);
}
// One 512-base chunk: the lane's dword (linearized), its valid bases, per base slot the match mask, wave prefix sum and chunk total; per
// tag the cursor before the chunk and pack = its 8-bit call mask | (its calls in the lanes below) << 8; U / H = the lane's / chunk's calls.
template <int NT, int NB> struct GeneralStep {
  uint32_t xl, vmask, m8[NB], incl[NB], cnt[NB], cur_before[NT], pack[NT], U, H;
};
template <int NT, int NB>
__device__ __forceinline__ void general_match_scan(GeneralStep<NT, NB>& S, const GeneralTags<NT, NB>& R, const ReadWalk& W, uint32_t x) {
  const uint32_t d = W.d0 + (uint32_t)lane_id();
  S.xl = linearize(x);
  S.vmask = (1u << min(max((int)W.L - (int)(8u * d), 0), 8)) - 1u;
  S.U = 0;
#pragma unroll
  for (int j = 0; j < NB; j++) {
    S.m8[j] = 0; S.incl[j] = 0; S.cnt[j] = 0;
    if ((uint32_t)j < R.nb) {
      S.m8[j] = match8(S.xl, (int)R.sbase[j]) & S.vmask; S.incl[j] = wave_incl_scan((uint32_t)__popc(S.m8[j]));
      S.cnt[j] = (uint32_t)__builtin_amdgcn_readlane((int)S.incl[j], 63);
      if ((R.implslots >> j) & 1u) S.U |= S.m8[j];
    }
  }
}
template <int NT, int NB>
__device__ __forceinline__ void general_mark_deposit(GeneralStep<NT, NB>& S, GeneralTags<NT, NB>& R, const ReadWalk& W, int n_tags,
    const MkpRunParams& prm, const uint32_t* __restrict__ ranks, uint32_t* __restrict__ ordb, const uint8_t* __restrict__ pdep4) {
  const uint32_t lane = (uint32_t)lane_id(), qa = 8u * W.d0, qb = min(qa + 512u, W.L);
  const bool rev = W.rev;
#pragma unroll
  for (int t = 0; t < NT; t++) { S.cur_before[t] = R.T.cur[t]; if (t < n_tags && lane < 18) ordb[t * 18 + lane] = 0; }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    if (t >= n_tags) break;
#ifdef MKP_DEBUG
    if (prm.debug_skip & 32u) break;   // ablation: no calls marked
#endif
    const bool any_base = R.desc[t].fb == 4;   // an `N` tag: ranks are positions
    const uint32_t sj = R.tslot[t];
    // window of ranks this chunk can ask for (windows of successive chunks tile the rank space); the bit marked is the chunk-relative
    // stored ordinal of the call's base, or its stored position
    const uint32_t first = any_base ? qa : selN<NB>(R.cum, sj), n = any_base ? qb - qa : selN<NB>(S.cnt, sj);
    const uint32_t tot = any_base ? W.L : selN<NB>(R.tot, sj);
    const uint32_t wlo = rev ? (tot - first - n) : first;
    mark_window(ranks, R.T.off[t], R.T.n[t], R.T.cur[t], rev, rank_batch(ranks, R.T.off[t], R.T.n[t], R.T.cur[t], rev), wlo, wlo + n, tot, first,
                ordb + t * 18);
  }
  wave_lds_sync();
#pragma unroll
  for (int t = 0; t < NT; t++) {
    S.pack[t] = 0;
    if (t < n_tags) {
      uint32_t bm;
      if (R.desc[t].fb == 4) bm = (ordb[t * 18 + (lane >> 2)] >> ((lane & 3) * 8)) & 0xffu & S.vmask;
      else {
        const uint32_t m = selN<NB>(S.m8, R.tslot[t]);
        bm = deposit_marks<8>(ordb + t * 18, pdep4, m, selN<NB>(S.incl, R.tslot[t]) - (uint32_t)__popc(m));
      }
      S.U |= bm; const uint32_t c2 = (uint32_t)__popc(bm); S.pack[t] = bm | ((wave_incl_scan(c2) - c2) << 8);
    }
  }
}
// every lane writes {lane, bit} of its called positions into the wave's slot list, in read order
template <int NT, int NB>
__device__ __forceinline__ void general_compact(GeneralStep<NT, NB>& S, uint16_t* __restrict__ slots) {
  const uint32_t ucnt = (uint32_t)__popc(S.U), uincl = wave_incl_scan(ucnt);
  S.H = (uint32_t)__builtin_amdgcn_readlane((int)uincl, 63);
  uint32_t ut = S.U, sidx = uincl - ucnt;
  while (ut) { slots[sidx++] = (uint16_t)(((uint32_t)lane_id() << 3) | ((uint32_t)__ffs((int)ut) - 1u)); ut &= ut - 1u; }
  wave_lds_sync();
}
// BaseModProbs of the lane's position (owner lane / bit of the chunk, base b) per mod strand: the tags that list it, in MM order
template <int NT, int NB>
__device__ __forceinline__ void general_position_probs(const GeneralStep<NT, NB>& S, const GeneralTags<NT, NB>& R, const MkpLayout* lay, int n_tags,
    bool rev, const uint8_t* __restrict__ ml, bool active, int owner, uint32_t bit, int x, int b, GState& S0, GState& S1, bool& err) {
#pragma unroll
  for (int k = 0; k < MKP_KMAX; k++) { at(S0.pk, k) = 0.f; at(S1.pk, k) = 0.f; }
  S0.H = S0.setmask = S1.H = S1.setmask = 0;
#pragma unroll
  for (int t = 0; t < NT; t++) {
    if (t >= n_tags) break;
    const MkpTagDesc dsc = R.desc[t];
    const uint32_t pt = __shfl(S.pack[t], owner, 64);
    if (!(active && ((pt >> bit) & 1u))) continue;
    if (x < 0) { err = true; continue; }  // a call listed on a non-ACGT base (DnaBase::try_from, mod_bam.rs:1245)
    const uint32_t idx = (pt >> 8) + (uint32_t)__popc(pt & ((1u << bit) - 1u));  // index among the tag's calls of this chunk, read order
    const uint32_t jx = rev ? (S.cur_before[t] - 1u - idx) : (S.cur_before[t] + idx);
    const uint32_t tm = lay->tagmap[t][b];  // [0:3] member index, [4+4i : 8+4i) local code of the tag's i-th code
    F4 ts = {0.f, 0.f, 0.f, 0.f};
    uint32_t seen = 0;
    for (int i = 0; i < (int)dsc.n_codes; i++) {   // as ml_prefetch / ml_to_probs, with a code the tag may list twice
      const float p = ((float)ml[R.T.ml[t] + jx * dsc.n_codes + i] + 0.5f) / 256.0f;
      const uint32_t kk = (tm >> (4 + 4 * i)) & 15u;
#pragma unroll
      for (int k = 0; k < MKP_KMAX; k++) if ((uint32_t)k == kk) {
        if (seen & (1u << k)) { if (at(ts, k) + p > 1.01f) err = true; at(ts, k) = at(ts, k) + p; } else { at(ts, k) = p; seen |= 1u << k; }
      }
    }
    if (merge_tag(dsc.neg ? S1 : S0, ts, seen, tm & 15u)) err = true;
  }
}
// The position's groups, '+' then '-' mod strand of base b: hit pattern, the tags behind it (contrib: 8 groups x 8 tag bits, for
// InvalidImplicitMode), classify_rule.  Up to two events; bit 12 marks the position's first.
template <bool SAMPLE>
__device__ __forceinline__ uint32_t general_classify(const MkpRunParams& prm, const uint8_t* __restrict__ bedmask, const uint32_t* lds_lay, int b,
    uint32_t aln, uint32_t L, bool trimmable, GState& S0, GState& S1, uint32_t f, bool mapped, int32_t rpos, ReadAcc& acc, uint32_t& contrib_lo,
    uint32_t& contrib_hi, uint32_t (&ev_info)[2], float (&sv)[2], int32_t& ev_pos) {
  uint32_t ev_cnt = 0;
#pragma unroll
  for (int sg = 0; sg < 2; sg++) {
    const int gi = sg * 4 + b;
    const uint32_t* gp = lds_lay + MKP_LAYOUT_GROUP_DW + gi * 32;
    const uint32_t gmisc = gp[0];
    if (MKP_G_NMEM(gmisc) == 0) continue;
    GState& S = sg ? S1 : S0;
    int pat; uint32_t members;
    if (!call_pattern(S.H, MKP_G_IMPL(gmisc), acc.err, pat, members)) continue;
    const GroupRegs gr = load_group(gp);
    const uint32_t tagbits = member_tagbits(members, gr.member_tags);
    if (gi < 4) contrib_lo |= tagbits << (8 * gi); else contrib_hi |= tagbits << (8 * (gi - 4));
    uint32_t info = 0; float v = 0.f;
    if (!classify_rule<SAMPLE>(prm, bedmask, gr, gp[12 + pat], MKP_KMAX, b, sg, aln, L, trimmable, pat == MKP_PAT_INFERRED, S.pk, f, mapped, rpos,
                               acc, info, v, ev_pos)) continue;
    if (ev_cnt) { ev_info[1] = info; sv[1] = v; } else { ev_info[0] = SAMPLE ? info : (info | (1u << 12)); sv[0] = v; }
    ev_cnt++;
  }
  return ev_cnt;
}

// NT = compile-time bound on the read's MM tag count (the entry point dispatches on it): loops and register arrays are sized for it.
template <bool SAMPLE, int NT>
__device__ __forceinline__ void decode_read_body(DECODE_PARAMS(const MkpRunParams&), uint32_t* __restrict__ lds_layouts,
    uint32_t (*__restrict__ lds_marks)[64], const uint8_t* __restrict__ pdep4) {
  const int lane = lane_id();
  uint32_t wib, rid; MkpReadHdr h; uint32_t* lds_lay;
  if (!read_prologue(hdrs, n_reads, read_ids, layouts, readout, lds_layouts, ~0u, wib, rid, h, lds_lay)) return;
  constexpr int NB = NT < 4 ? NT : 4;   // distinct stored bases the tags can count
  uint32_t* __restrict__ ordb = &lds_marks[wib * 7][0];                        // [NT][18] ordinal / position bitmaps of the chunk
  uint16_t* __restrict__ slots = reinterpret_cast<uint16_t*>(ordb + 192);                 // 512 compacted {lane, bit} entries
  const MkpLayout* lay = reinterpret_cast<const MkpLayout*>(lds_lay);
  const int n_tags = (int)h.n_tags;
  ReadWalk W; W.seqw = reinterpret_cast<const uint32_t*>(seqs + h.seq_off); W.L = h.l_seq; W.nd = (W.L + 7u) >> 3; W.rev = (h.flags & MKP_RF_REVERSE) != 0;
  const bool rev = W.rev; const uint32_t L = W.L, aln = rev ? 1u : 0u;
  GeneralTags<NT, NB> R; tag_lists<NT>(tagref, h.tag_off, n_tags, rev, R.T);
  general_base_slots(R, lay, lds_lay, n_tags, rev);
  if (rev) {
#pragma unroll
    for (int j = 0; j < NB; j++) if ((uint32_t)j < R.nb) R.tot[j] = stored_base_total(W.seqw, W.nd, L, (int)R.sbase[j]);
  }
  ReadAcc acc; bool& err = acc.err;
  const bool trimmable = read_trimmable(prm, L);
  uint32_t contrib_lo = 0, contrib_hi = 0;
  uint32_t x_next = (uint32_t)lane < W.nd ? W.seqw[lane] : 0u;   // the next step's SEQ dword is always in flight
  CigarWin win; win.wr0 = h.ref_start;

  for (; W.d0 < W.nd && !err; W.d0 += 64) {
    GeneralStep<NT, NB> S;
    general_match_scan(S, R, W, x_next);
    { const uint32_t dn = W.d0 + 64u + (uint32_t)lane; x_next = dn < W.nd ? W.seqw[dn] : 0u; }
    general_mark_deposit(S, R, W, n_tags, prm, ranks, ordb, pdep4);
    general_compact(S, slots);
    for (uint32_t g0 = 0; g0 < S.H && !err; g0 += 64) {   // the called positions, 64 per batch, in read order
#ifdef MKP_DEBUG
      if (prm.debug_skip & 16u) break;   // ablation: producer only
#endif
      const bool active = g0 + lane < S.H;
      const uint32_t slot = active ? (uint32_t)slots[g0 + lane] : 0u;
      const int owner = (int)(slot >> 3);
      const uint32_t bit = slot & 7u, q = 8u * (W.d0 + (uint32_t)owner) + bit;
      const uint32_t xo = __shfl(S.xl, owner, 64);   // from every lane: an owner may be inactive in the chunk's last batch
      const int x = active ? nib2base((xo >> (4u * bit)) & 15u) : -1;
      const uint32_t f = rev ? (L - 1 - q) : q;  // forward (as-sequenced) position
      const int b = x < 0 ? -1 : (rev ? 3 - x : x);
      GState S0, S1;
      general_position_probs(S, R, lay, n_tags, rev, ml, active, owner, bit, x, b, S0, S1, err);
      bool mapped = false; int32_t rpos = 0;
      cigar_map(win, h, cigar, active && x >= 0, q, mapped, rpos);
      uint32_t ev_info[2]; float sv[2] = {0.f, 0.f}; uint32_t ev_cnt = 0; int32_t ev_pos = SAMPLE ? 0 : rpos;
      if (active && x >= 0)
        ev_cnt = general_classify<SAMPLE>(prm, bedmask, lds_lay, b, aln, L, trimmable, S0, S1, f, mapped, rpos, acc, contrib_lo, contrib_hi,
                                          ev_info, sv, ev_pos);
      append_events<SAMPLE, 2>(events, sample_vals, dev_err, h.event_off, h.event_cap, ev_cnt, (uint32_t)ev_pos, ev_info, sv, acc);
      err = __any(err);
    }
#pragma unroll
    for (int j = 0; j < NB; j++) R.cum[j] += S.cnt[j];
    err = __any(err);
  }
#pragma unroll
  for (int t = 0; t < NT; t++) if (t < n_tags && list_left_over(rev, R.T.cur[t], R.T.n[t])) err = true;
  if (!prm.force_allow && !SAMPLE) {   // InvalidImplicitMode, per group
    contrib_lo = wave_or(contrib_lo); contrib_hi = wave_or(contrib_hi);
    for (int gi = 0; gi < 8; gi++)
      if (lacks_mode(((gi < 4 ? contrib_lo >> (8 * gi) : contrib_hi >> (8 * (gi - 4)))) & 0xffu, lay->default_mask)) err = true;
  }
  read_epilogue(readout, rid, acc, false);
}

// ----------------------------------------------------------------------------------------------
// The single-group decoders, FAST and SPARSE: a producer/consumer inside the wave.  The producer's steps only *locate* calls and append
// {stored position, ML call index per tag} to a queue in LDS (SoA columns); whenever 64 calls are queued consume_batch runs the per-call
// work on a full batch (a 1024-base step of CpG data finds ~13 calls).  Group descriptor, thresholds, code maps: wave-uniform (SGPRs).
// The one (mod strand, base) group of the decoder's tags tb .. tb+n_tags: descriptor (words at gp), stored base counted, the
// tags' constants (tag_setup), and the hit pattern / code set of a call that every tag lists.  Wave-uniform.
template <int NT> struct GroupCalls {
  GroupRegs g; const uint32_t* gp; int b0, sg0, xs; uint32_t kcodes, impl, SH_all, setmask_all;
  uint32_t t_nc[NT], tmu[NT], codes_t[NT];
};
template <int NT>
__device__ __forceinline__ void group_setup(const MkpLayout* lay, const uint32_t* lds_lay, int tb, int n_tags, bool rev, GroupCalls<NT>& G) {
  G.b0 = (int)lay->tags[tb].fb & 3; G.sg0 = (int)lay->tags[tb].neg & 1;
  G.xs = rev ? 3 - G.b0 : G.b0;
  G.gp = lds_lay + MKP_LAYOUT_GROUP_DW + (G.sg0 * 4 + G.b0) * 32;
  G.g = load_group_uniform(G.gp);
  G.impl = MKP_G_IMPL(G.g.misc);
  G.kcodes = (G.g.misc >> 20) & 7u;   // codes of the group: bounds every per-code loop
  tag_setup<NT>(lay, tb, n_tags, G.b0, G.t_nc, G.tmu, G.codes_t);
  G.SH_all = 0; G.setmask_all = 0;
#pragma unroll
  for (int t = 0; t < NT; t++) if (t < n_tags) { G.SH_all |= 1u << (G.tmu[t] & 15u); G.setmask_all |= G.codes_t[t]; }
}
// where a read's events go: its slice of the event list
struct EventSink { MkpEvent* __restrict__ events; float* __restrict__ sample_vals; uint32_t* __restrict__ dev_err; uint32_t ev_base, ev_cap; };

// Consumer: up to 64 queued calls, in read order, one per lane: ml_prefetch, CIGAR mapping (map_window on the decoder's window),
// ml_to_probs, classify_call, append_events.  q_j[t] = the queue column holding tag t's ML call index.  INFER: the group may
// have implicit-mode members and a tag may not list a call (index ~0); else every tag lists every call and never infers.
template <bool SAMPLE, bool INFER, int NT, class Win>
__device__ __forceinline__ void consume_batch(const MkpRunParams& prm, const uint8_t* __restrict__ bedmask, const uint8_t* __restrict__ ml,
    const GroupCalls<NT>& G, const uint32_t (&t_ml)[NT], int n_tags, const ReadWalk& W, bool trimmable, const uint32_t* __restrict__ q_pos,
    uint32_t* const (&q_j)[NT], uint32_t& qhead, uint32_t qcount, Win& win, const MkpReadHdr& h, const uint32_t* __restrict__ cigar,
    const EventSink& out, ReadAcc& acc, uint32_t& contribH) {
  const uint32_t lane = (uint32_t)lane_id(), nb = min(64u, qcount - qhead);
  const bool active = lane < nb;
  const uint32_t q = active ? q_pos[qhead + lane] : 0u;
  const uint32_t f = W.rev ? (W.L - 1 - q) : q;  // forward (as-sequenced) position
  uint32_t mlq[NT][MKP_KMAX], jx[NT]; bool found[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    if (INFER) { jx[t] = (t < n_tags && active) ? q_j[t][qhead + lane] : 0xffffffffu; found[t] = jx[t] != 0xffffffffu; }
    else { jx[t] = active ? q_j[t][qhead + lane] : 0u; found[t] = active; }
  }
  ml_prefetch<NT>(ml, n_tags, t_ml, G.t_nc, found, jx, mlq);
  bool mapped = false; int32_t rpos = 0;
#ifdef MKP_DEBUG
  if (!INFER && (prm.debug_skip & 32u)) { mapped = active; rpos = h.ref_start + (int32_t)q; } else   // ablation: no CIGAR mapping
#endif
  map_window<SAMPLE>(win, h, cigar, active, q, mapped, rpos);
  F4 pk = {0.f, 0.f, 0.f, 0.f};
  uint32_t SH = G.SH_all, setmask = G.setmask_all;   // the members whose tags list the call, their local codes
  bool check = active && n_tags > 1;
  if (INFER) {
    SH = 0; setmask = 0;
#pragma unroll
    for (int t = 0; t < NT; t++) { SH |= found[t] ? (1u << (G.tmu[t] & 15u)) : 0u; setmask |= found[t] ? G.codes_t[t] : 0u; }
    check = __popc(SH) >= 2;
  }
  if (ml_to_probs<NT>(mlq, n_tags, G.t_nc, G.tmu, found, setmask, check, pk)) acc.err = true;
  uint32_t ev_info[1] = {0}; float sv[1] = {0.f}; bool has_ev = false;
  if (active && (!INFER || (SH | G.impl)))
    has_ev = classify_call<SAMPLE, INFER>(prm, bedmask, G.g, G.gp, (int)G.kcodes, G.b0, G.sg0, W.rev ? 1u : 0u, W.L, trimmable, SH, G.impl, pk, f,
                                          mapped, rpos, acc, contribH, ev_info[0], sv[0]);
  append_events<SAMPLE, 1>(out.events, out.sample_vals, out.dev_err, out.ev_base, out.ev_cap, has_ev ? 1u : 0u, (uint32_t)rpos, ev_info, sv, acc);
  acc.err = __any(acc.err);
  qhead += nb;
}
// InvalidImplicitMode of the one group, once the read is walked
template <bool SAMPLE, int NT>
__device__ __forceinline__ void group_epilogue(const MkpRunParams& prm, const MkpLayout* lay, const GroupCalls<NT>& G, uint32_t contribH,
    ReadAcc& acc) {
  if (!prm.force_allow && !SAMPLE && lacks_mode(member_tagbits(wave_or(contribH), G.g.member_tags), lay->default_mask)) acc.err = true;
}

// ----------------------------------------------------------------------------------------------
// Decode, FAST layouts (MkpLayout::fast: every tag on the same specific base and mod strand, no code listed twice —
// `C+m?`, `C+hm?`, `C+h?;C+m?`, ...; NT <= 2 tags).  Same semantics as decode_read_body.  1024-base steps, 16 bases per lane:
//   fast_locate_step    match mask and wave scan of the counted base, the tags' ranks of the step's window marked in the ordinal
//                       bitmap and deposited onto the match mask, scan of the union (plus every occurrence for implicit members);
//   fast_append_half    the located calls go to the queue in two halves (lanes 0-31, then 32-63), so that the queue never has
//                       to take more than 512 entries at once;
//   consume_batch<INFER = true>.
#define MKP_QCAP 576   // 63 left over + up to 512 from half a step (32 lanes x 16 bases)
#define MKP_ORD_WORDS 34   // ordinal bitmap of a 1024-base step: 32 words + 2 for the 64-bit window read
template <int NT> struct FastStep {
  uint32_t xn0, xn1;                      // the next step's SEQ dwords (two per lane), always in flight
  bool pend = false;                      // the located step's upper lanes still hold calls
  uint32_t cntT = 0;                      // occurrences of the base in the step
  uint32_t U = 0, uexcl = 0;              // the lane's calls (bit per base), the calls of the lanes below
  uint32_t H = 0, HA = 0;                 // calls of the step, of its lanes 0-31
  uint32_t bm[NT], texcl[NT], cur[NT];    // per tag: the lane's listed calls, those of the lanes below, the cursor before the step
};
template <int NT>
__device__ __forceinline__ void fast_fetch_seq(FastStep<NT>& S, const ReadWalk& W, uint32_t dstep) {
  const uint32_t d = dstep + 2u * (uint32_t)lane_id();
  S.xn0 = d < W.nd ? W.seqw[d] : 0u; S.xn1 = d + 1u < W.nd ? W.seqw[d + 1u] : 0u;
}
template <int NT>
__device__ __forceinline__ void fast_locate_step(FastStep<NT>& S, const ReadWalk& W, TagLists<NT>& T, int n_tags, int xs, bool implicit,
    const uint32_t* __restrict__ ranks, uint32_t* __restrict__ ordb, const uint8_t* __restrict__ pdep4) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t d = W.d0 + 2u * lane;          // this lane's first dword: bases [8d, 8d+16)
  const uint32_t xl0 = linearize(S.xn0), xl1 = linearize(S.xn1);
  fast_fetch_seq(S, W, W.d0 + 128u);
  // the first 64 ranks at every tag's cursor are requested now, ahead of the match/scan work that decides how many are used
  RankBatch pre[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) { pre[t].e = 0; pre[t].valid = false; if (t < n_tags) pre[t] = rank_batch(ranks, T.off[t], T.n[t], T.cur[t], W.rev); }
  const int nv = min(max((int)W.L - (int)(8u * d), 0), 16);
  const uint32_t m16 = (match8(xl0, xs) | (match8(xl1, xs) << 8)) & ((1u << nv) - 1u);
  const uint32_t c = (uint32_t)__popc(m16), incl = wave_incl_scan(c);
  const uint32_t cntT = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  const uint32_t wlo = W.rev ? (W.tot - W.cum - cntT) : W.cum, whi = wlo + cntT;   // rank window of this step
#pragma unroll
  for (int t = 0; t < NT; t++) { S.cur[t] = T.cur[t]; if (t < n_tags && lane < MKP_ORD_WORDS) ordb[t * MKP_ORD_WORDS + lane] = 0; }
#pragma unroll
  for (int t = 0; t < NT; t++)
    if (t < n_tags) mark_window(ranks, T.off[t], T.n[t], T.cur[t], W.rev, pre[t], wlo, whi, W.tot, W.cum, ordb + t * MKP_ORD_WORDS);
  wave_lds_sync();
  uint32_t U = implicit ? m16 : 0u, uincl = 0, ucnt = 0;
#pragma unroll
  for (int t = 0; t < NT; t++) {
    S.bm[t] = 0; S.texcl[t] = 0;
    if (t < n_tags) {
      S.bm[t] = deposit_marks<16>(ordb + t * MKP_ORD_WORDS, pdep4, m16, incl - c);
      U |= S.bm[t];
      const uint32_t c2 = (uint32_t)__popc(S.bm[t]);
      uincl = wave_incl_scan(c2); ucnt = c2; S.texcl[t] = uincl - c2;
    }
  }
  if (NT > 1 || implicit) { ucnt = (uint32_t)__popc(U); uincl = wave_incl_scan(ucnt); }   // else U == bm[0]: its scan is already there
  S.U = U; S.uexcl = uincl - ucnt; S.cntT = cntT;
  S.H = (uint32_t)__builtin_amdgcn_readlane((int)uincl, 63); S.HA = (uint32_t)__builtin_amdgcn_readlane((int)uincl, 31);
}
// append one half's calls: lanes 0-31 first, lanes 32-63 on the next visit; the step is done when no half is left
template <int NT>
__device__ __forceinline__ void fast_append_half(FastStep<NT>& S, ReadWalk& W, uint32_t* __restrict__ q_pos, uint32_t* const (&q_j)[NT],
    uint32_t& qcount) {
  const bool mine = S.pend ? (lane_id() >= 32) : (lane_id() < 32);
  const uint32_t d = W.d0 + 2u * (uint32_t)lane_id();   // the lane's first dword, as the step was located
  uint32_t ut = mine ? S.U : 0u, sidx = qcount + S.uexcl - (S.pend ? S.HA : 0u);
  while (ut) {
    const uint32_t bit = (uint32_t)__ffs((int)ut) - 1u, below = (1u << bit) - 1u;
    q_pos[sidx] = 8u * d + bit;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const uint32_t idx = S.texcl[t] + (uint32_t)__popc(S.bm[t] & below);
      const uint32_t jx = W.rev ? (S.cur[t] - 1u - idx) : (S.cur[t] + idx);
      q_j[t][sidx] = ((S.bm[t] >> bit) & 1u) ? jx : 0xffffffffu;
    }
    sidx++; ut &= ut - 1u;
  }
  wave_lds_sync();
  qcount += S.pend ? (S.H - S.HA) : S.HA;
  if (!S.pend && S.H > S.HA) S.pend = true;
  else { S.pend = false; W.cum += S.cntT; W.d0 += 128; }
}

template <bool SAMPLE, int NT>
__device__ __forceinline__ void decode_read_fast(DECODE_PARAMS(const MkpRunParams&), uint32_t* __restrict__ lds_layouts,
    uint32_t* __restrict__ lds_ord, const uint8_t* __restrict__ pdep4, uint32_t* __restrict__ lds_queue) {
  static_assert(NT <= 2, "the call queue holds two ML indices per entry");
  uint32_t wib, rid; MkpReadHdr h; uint32_t* lds_lay;
  if (!read_prologue(hdrs, n_reads, read_ids, layouts, readout, lds_layouts, ~0u, wib, rid, h, lds_lay)) return;
  uint32_t* __restrict__ ordb = lds_ord + wib * (NT * MKP_ORD_WORDS);   // [NT][MKP_ORD_WORDS] ordinal bitmaps of the step
  // queue, SoA: stored position, ML call index of tag 0 / 1 (~0 = not listed)
  uint32_t* __restrict__ q_pos = lds_queue + wib * ((1 + NT) * MKP_QCAP);
  uint32_t* q_j[NT];
  for (int t = 0; t < NT; t++) q_j[t] = q_pos + (1 + t) * MKP_QCAP;
  const MkpLayout* lay = reinterpret_cast<const MkpLayout*>(lds_lay);
  const int n_tags = (int)h.n_tags;
  ReadWalk W; W.seqw = reinterpret_cast<const uint32_t*>(seqs + h.seq_off); W.L = h.l_seq; W.nd = (W.L + 7u) >> 3; W.rev = (h.flags & MKP_RF_REVERSE) != 0;
  GroupCalls<NT> G; group_setup<NT>(lay, lds_lay, 0, n_tags, W.rev, G);
  TagLists<NT> T; tag_lists<NT>(tagref, h.tag_off, n_tags, W.rev, T);
  if (W.rev) W.tot = stored_base_total(W.seqw, W.nd, W.L, G.xs);
  ReadAcc acc;
  const bool trimmable = read_trimmable(prm, W.L);
  const EventSink out = {events, sample_vals, dev_err, h.event_off, h.event_cap};
  uint32_t contribH = 0, qhead = 0, qcount = 0;
  CigarWin win; win.wr0 = h.ref_start;
  FastStep<NT> S; fast_fetch_seq(S, W, 0);
  for (int t = 0; t < NT; t++) { S.bm[t] = 0; S.texcl[t] = 0; S.cur[t] = 0; }

  while (!acc.err) {
    if (qcount - qhead < 64u && (S.pend || W.d0 < W.nd)) {   // producer
      if (qhead) queue_to_front<1 + NT>(q_pos, MKP_QCAP, qhead, qcount);
      if (!S.pend) fast_locate_step(S, W, T, n_tags, G.xs, G.impl != 0u, ranks, ordb, pdep4);
      fast_append_half(S, W, q_pos, q_j, qcount);
      continue;
    }
    if (qcount == qhead) break;
#ifdef MKP_DEBUG
    if (prm.debug_skip & 16u) { qhead = qcount; continue; }   // ablation: producer only
#endif
    consume_batch<SAMPLE, true, NT>(prm, bedmask, ml, G, T.ml, n_tags, W, trimmable, q_pos, q_j, qhead, qcount, win, h, cigar, out, acc, contribH);
  }
#pragma unroll
  for (int t = 0; t < NT; t++) if (t < n_tags && list_left_over(W.rev, T.cur[t], T.n[t])) acc.err = true;
  group_epilogue<SAMPLE, NT>(prm, lay, G, contribH, acc);
  read_epilogue(readout, rid, acc, false);
}

// ----------------------------------------------------------------------------------------------
// Decode, SPARSE layouts: FAST layouts whose tags are all explicit ('?': only the listed bases are calls) and, when there are
// two tags, list the same bases (`C+h?,..;C+m?,..` with one delta list — checked by the host).  The calls are then a few
// percent of the bases, and locating them must not cost per base.  4096-base steps, 64 bases = 8 SEQ dwords per lane:
//   sparse_count_step   the wave only counts: per dword a nibble-equality flag word (7 VALU for 8 bases) and its popcount,
//                       byte-packed running counts inside the lane, one wave prefix sum; the flag words go to LDS;
//   sparse_locate       the window's ranks are taken 64 at a time from the sorted list; every lane owning one finds the lane whose
//                       bases contain that occurrence (6 ds_bpermute steps over the prefix sums), the dword inside that lane (one SWAR
//                       compare over the packed counts) and the base inside the dword (select on the flag word read back from LDS) —
//                       {stored position, call index} goes straight into the queue, in read order.  No per-base marks, no deposit;
//   consume_batch<INFER = false>: "every tag lists every call, no implicit members", on descriptor words made opaque per batch and
//                       with a CIGAR window of the decoder's own (PairWin: 128 ops, scalar running values).
#define MKP_SQCAP 128   // call queue of the SPARSE kernels: < 64 left over + one round of <= 64
struct SparseStep {
  uint4 xa, xb;                 // the next step's SEQ dwords (eight per lane, two 16-byte loads), always in flight
  bool loaded = false;          // the step below is counted and still holds ranks
  uint32_t incl = 0, excl = 0;  // wave prefix sums of the lanes' counts
  uint32_t cumlo = 0, cumhi = 0;   // byte-packed exclusive running counts of the lane's 8 dwords
  uint32_t cntT = 0, wlo = 0, whi = 0;   // occurrences in the step, its rank window
};
// SEQ buffers end with slack, so whole vectors are loaded and the dwords past the read are discarded here; reads start 4-byte
// aligned: vector loads may be unaligned (fine on global memory)
__device__ __forceinline__ void sparse_fetch_seq(SparseStep& S, const ReadWalk& W, uint32_t dstep) {
  const uint32_t d = dstep + 8u * (uint32_t)lane_id(), nd = W.nd; const uint32_t* __restrict__ seqw = W.seqw;
  if (d + 4u <= nd) S.xa = *reinterpret_cast<const uint4*>(seqw + d);
  else { S.xa.x = d < nd ? seqw[d] : 0u; S.xa.y = d + 1u < nd ? seqw[d + 1u] : 0u; S.xa.z = d + 2u < nd ? seqw[d + 2u] : 0u; S.xa.w = 0u; }
  if (d + 8u <= nd) S.xb = *reinterpret_cast<const uint4*>(seqw + d + 4u);
  else { S.xb.x = d + 4u < nd ? seqw[d + 4u] : 0u; S.xb.y = d + 5u < nd ? seqw[d + 5u] : 0u; S.xb.z = d + 6u < nd ? seqw[d + 6u] : 0u; S.xb.w = 0u; }
}
__device__ __forceinline__ void sparse_count_step(SparseStep& S, const ReadWalk& W, uint32_t pat, const OddTail& odd, uint32_t* __restrict__ flg) {
  const uint32_t lane = (uint32_t)lane_id(), d = W.d0 + 8u * lane;          // this lane's first dword: bases [8d, 8d+64)
  uint32_t F[8] = {nibble_eq(S.xa.x, pat), nibble_eq(S.xa.y, pat), nibble_eq(S.xa.z, pat), nibble_eq(S.xa.w, pat),
                   nibble_eq(S.xb.x, pat), nibble_eq(S.xb.y, pat), nibble_eq(S.xb.z, pat), nibble_eq(S.xb.w, pat)};
  if (odd.dw - d < 8u) {   // the read's last dword sits in this lane and L is odd
#pragma unroll
    for (int j = 0; j < 8; j++) if (d + (uint32_t)j == odd.dw) F[j] &= odd.clear;
  }
  sparse_fetch_seq(S, W, W.d0 + 512u);
  __builtin_amdgcn_wave_barrier();   // the previous step's readers of the flag words are done (same wave: program order)
  *reinterpret_cast<uint4*>(flg + 8u * lane) = make_uint4(F[0], F[1], F[2], F[3]);
  *reinterpret_cast<uint4*>(flg + 8u * lane + 4u) = make_uint4(F[4], F[5], F[6], F[7]);
  // byte-packed counts, then running counts inside the lane (byte k = count of the dwords before k)
  const uint32_t clo = (uint32_t)__popc(F[0]) | ((uint32_t)__popc(F[1]) << 8) | ((uint32_t)__popc(F[2]) << 16) | ((uint32_t)__popc(F[3]) << 24);
  const uint32_t chi = (uint32_t)__popc(F[4]) | ((uint32_t)__popc(F[5]) << 8) | ((uint32_t)__popc(F[6]) << 16) | ((uint32_t)__popc(F[7]) << 24);
  const uint32_t plo = clo + (clo << 8) + (clo << 16) + (clo << 24);   // inclusive prefix per byte (sums stay below 256)
  const uint32_t tlo = plo >> 24;                                     // count of dwords 0..3
  const uint32_t phi = chi + (chi << 8) + (chi << 16) + (chi << 24) + tlo * 0x01010101u;
  S.cumlo = plo << 8; S.cumhi = (phi << 8) | tlo;                      // exclusive
  const uint32_t c = phi >> 24;                                       // the lane's 64 bases
  S.incl = wave_incl_scan(c); S.excl = S.incl - c;
  S.cntT = (uint32_t)__builtin_amdgcn_readlane((int)S.incl, 63);
  S.wlo = W.rev ? (W.tot - W.cum - S.cntT) : W.cum; S.whi = S.wlo + S.cntT;   // rank window of this step
  S.loaded = true;
  wave_lds_sync();
}
// stored position of the lane's taken rank e
__device__ __forceinline__ uint32_t sparse_locate(const SparseStep& S, const ReadWalk& W, bool hit, uint32_t e, const uint32_t* __restrict__ flg) {
  const uint32_t ib = hit ? step_ordinal(e, W.rev, W.tot, W.cum) : 0u;    // step-relative stored ordinal of the called base (< cntT)
  const int owner = find_op(S.incl, ib) & 63;                             // the lane whose 64 bases hold that occurrence
  const uint32_t o_excl = (uint32_t)__shfl((int)S.excl, owner, 64), o_lo = (uint32_t)__shfl((int)S.cumlo, owner, 64),
      o_hi = (uint32_t)__shfl((int)S.cumhi, owner, 64);
  const uint32_t k = ib - o_excl;                                         // occurrence inside the owner's 64 bases
  // dword: the last of the 8 running counts that is <= k (SWAR: byte i of t keeps 0x80 where count_i > k; counts < 128)
  const uint32_t kk1 = (k + 1u) * 0x01010101u;
  const uint32_t t_lo = ((o_lo | 0x80808080u) - kk1) & 0x80808080u, t_hi = ((o_hi | 0x80808080u) - kk1) & 0x80808080u;
  const uint32_t jd = 7u - (uint32_t)__popc(t_lo) - (uint32_t)__popc(t_hi);
  const uint32_t cj = ((jd < 4u ? o_lo : o_hi) >> (8u * (jd & 3u))) & 0xffu;
  uint32_t r = k - cj;
  uint32_t Fw = hit ? flg[8u * (uint32_t)owner + jd] : 1u;
  Fw = ((Fw & 0x01010101u) << 4) | ((Fw >> 4) & 0x01010101u);           // base order: bit 4b = base b of the dword
  uint32_t bpos = 0, cc;
  cc = (uint32_t)__popc(Fw & 0xffffu); if (r >= cc) { r -= cc; bpos += 4u; Fw >>= 16; }
  cc = (uint32_t)__popc(Fw & 0xffu);   if (r >= cc) { r -= cc; bpos += 2u; Fw >>= 8; }
  cc = Fw & 1u;                         if (r >= cc) { bpos += 1u; }
  return 8u * (W.d0 + 8u * (uint32_t)owner + jd) + bpos;
}

// Query -> reference through the SPARSE decoder's own CIGAR window, advanced as the batches move along the read.  128 ops per window,
// two per lane: qe = inclusive query end of the lane's pair, mid = where its second op starts, a / b = (reference start - query
// start) << 1 | is-match of the two ops.  The running values (first op, query / reference offsets, totals) are kept in scalar registers,
// read back through readfirstlane after every update (as vectors they were advanced with v_cndmask and copied at every loop head);
// "nothing loaded yet" is an empty window in front of op 0: no flag, no conditional advance (as the slot walks' CigarWin, mkp_slots.hip).
struct PairWin {
  uint32_t c0 = 0u - 128u, wq0 = 0, wq1 = 0; int32_t wr0; uint32_t rtot = 0;
  uint32_t qe = 0, mid = 0, a = 0, b = 0;
  uint2 pref;   // the next window's ops, requested one window ahead: the load is off the mapping's dependency chain
};
__device__ __forceinline__ uint2 pairwin_fetch(const MkpReadHdr& h, const uint32_t* __restrict__ cigar, uint32_t c) {
  uint2 r; const uint32_t k = c + 2u * (uint32_t)lane_id();
  r.x = k < h.n_cigar ? cigar[h.cigar_off + k] : 5u /*0H*/; r.y = k + 1u < h.n_cigar ? cigar[h.cigar_off + k + 1u] : 5u;
  return r;
}
// the next 128 ops; false behind the last op (cannot happen for positions inside SEQ: the packer checks the lengths)
__device__ __forceinline__ bool pairwin_next(PairWin& w, const MkpReadHdr& h, const uint32_t* __restrict__ cigar) {
  w.c0 = rfl_u(w.c0 + 128u); w.wq0 = w.wq1; w.wr0 = (int32_t)rfl_u((uint32_t)w.wr0 + w.rtot);
  if (w.c0 >= h.n_cigar) { w.rtot = 0; return false; }
  const uint2 p = w.pref;
  w.pref = pairwin_fetch(h, cigar, w.c0 + 128u);
  const uint32_t op0 = p.x & 15u, len0 = p.x >> 4, op1 = p.y & 15u, len1 = p.y >> 4;
  const uint32_t ql0 = op_consumes_query(op0) ? len0 : 0u, rl0 = op_consumes_ref(op0) ? len0 : 0u;
  const uint32_t ql1 = op_consumes_query(op1) ? len1 : 0u, rl1 = op_consumes_ref(op1) ? len1 : 0u;
  w.qe = wave_incl_scan(ql0 + ql1); const uint32_t re = wave_incl_scan(rl0 + rl1);
  w.mid = w.qe - ql1;                                                       // window-relative query offset of the second op
  const int32_t dl0 = (w.wr0 + (int32_t)(re - rl0 - rl1)) - (int32_t)(w.wq0 + w.qe - ql0 - ql1);   // ref start - query start of the first op
  const int32_t dl1 = (w.wr0 + (int32_t)(re - rl1)) - (int32_t)(w.wq0 + w.mid);
  w.a = ((uint32_t)dl0 << 1) | (op_is_match(op0) ? 1u : 0u); w.b = ((uint32_t)dl1 << 1) | (op_is_match(op1) ? 1u : 0u);
  w.wq1 = w.wq0 + (uint32_t)__builtin_amdgcn_readlane((int)w.qe, 63); w.rtot = (uint32_t)__builtin_amdgcn_readlane((int)re, 63);
  return true;
}
// the lanes whose position lies in the loaded window (positions ascend from batch to batch: none lies before it)
__device__ __forceinline__ void pairwin_pass(const PairWin& w, bool& pending, uint32_t q, bool& mapped, int32_t& rpos) {
  const bool ready = pending && q < w.wq1;
  if (!__any(ready)) return;
  const uint32_t qrel = ready ? q - w.wq0 : 0u;
  const int oi = find_op(w.qe, qrel) & 63;
  const uint32_t o_mid = (uint32_t)__shfl((int)w.mid, oi, 64), o_a = (uint32_t)__shfl((int)w.a, oi, 64), o_b = (uint32_t)__shfl((int)w.b, oi, 64);
  const uint32_t pick = qrel < o_mid ? o_a : o_b;
  if (ready) { mapped = (pick & 1u) != 0u; rpos = (int32_t)q + ((int32_t)pick >> 1); pending = false; }
}
// BY_VALUE: the window is copied in, advanced and copied back.  The sample kernels, which have no launch bound, keep their eighth wave
// only in this form (behind the reference 65 VGPRs for 57 / 63); the event kernels are faster behind the reference
// (profiles/decoder_stages_isa.txt, decoder_stages_ab.txt).
template <bool BY_VALUE>
__device__ __forceinline__ void pairwin_map(PairWin& win, const MkpReadHdr& h, const uint32_t* __restrict__ cigar, bool pending, uint32_t q,
    bool& mapped, int32_t& rpos) {
  PairWin copy; if (BY_VALUE) copy = win;
  PairWin& w = BY_VALUE ? copy : win;
  pairwin_pass(w, pending, q, mapped, rpos);
  while (__any(pending)) { if (!pairwin_next(w, h, cigar)) break; pairwin_pass(w, pending, q, mapped, rpos); }
  if (BY_VALUE) win = copy;
}
template <bool SAMPLE>
__device__ __forceinline__ void map_window(PairWin& w, const MkpReadHdr& h, const uint32_t* __restrict__ cigar, bool pending, uint32_t q,
    bool& mapped, int32_t& rpos) { pairwin_map<SAMPLE>(w, h, cigar, pending, q, mapped, rpos); }

template <bool SAMPLE, int NT>
__device__ __forceinline__ void decode_read_sparse(DECODE_PARAMS(const MkpRunParams&), uint32_t* __restrict__ lds_layouts,
    uint32_t* __restrict__ lds_queue, uint32_t* __restrict__ lds_flags) {
  static_assert(NT <= 2, "one or two tags");
  const uint32_t lane = (uint32_t)lane_id();
  // Duplex reads (layout.fast == 2: two (strand, base) groups on different bases) are listed twice, once per group (bit 31 = the
  // second); each listing decodes its group's tags exactly like a single-group read, into its own half of the read's event slice
  // behind the room for the merged list, with its own summary; mkp_merge_duplex interleaves the two by position afterwards.
  uint32_t wib, rid_raw; MkpReadHdr h; uint32_t* lds_lay;
  if (!read_prologue(hdrs, n_reads, read_ids, layouts, readout, lds_layouts, 0x7fffffffu, wib, rid_raw, h, lds_lay)) return;
  const uint32_t rid = rid_raw & 0x7fffffffu; const bool half_b = (rid_raw >> 31) != 0u;
  uint32_t* __restrict__ q_pos = lds_queue + wib * (2 * MKP_SQCAP);   // queue, SoA: stored position, call index (the same for both tags)
  uint32_t* __restrict__ q_idx = q_pos + MKP_SQCAP;
  uint32_t* q_j[NT];
  for (int t = 0; t < NT; t++) q_j[t] = q_idx;
  uint32_t* __restrict__ flg = lds_flags + wib * 512u;                 // the step's 512 flag words
  const MkpLayout* lay = reinterpret_cast<const MkpLayout*>(lds_lay);
  ReadWalk W; W.seqw = reinterpret_cast<const uint32_t*>(seqs + h.seq_off); W.L = h.l_seq; W.nd = (W.L + 7u) >> 3; W.rev = (h.flags & MKP_RF_REVERSE) != 0;
  const bool rev = W.rev, duplex = rfl_u(lay->fast) == 2u;
  const int n_first = (int)rfl_u(lay->pad);
  const int tb = (duplex && half_b) ? n_first : 0;                     // first tag of the group this wave decodes
  const int n_tags = duplex ? (half_b ? (int)h.n_tags - n_first : n_first) : (int)h.n_tags;
  EventSink out = {events, sample_vals, dev_err, h.event_off, h.event_cap};
  uint32_t ro_idx = rid;
  if (duplex) {
    const uint32_t nA = tagref[h.tag_off].n, nB = tagref[h.tag_off + n_first].n;   // calls listed per group (one shared rank list each)
    out.ev_base = h.event_off + nA + nB + (half_b ? nA : 0u); out.ev_cap = half_b ? nB : nA;
    if (half_b) ro_idx = prm.readout_b_off + rid;
  }
  GroupCalls<NT> G; group_setup<NT>(lay, lds_lay, tb, n_tags, rev, G);
  TagLists<NT> T; tag_lists<NT>(tagref, h.tag_off + tb, n_tags, rev, T);   // list 0 is the shared one
  const uint32_t pat = 0x11111111u << G.xs;
  const OddTail odd = odd_tail(W.L);
  if (rev) W.tot = stored_base_total(W.seqw, W.nd, W.L, G.xs);
  ReadAcc acc;
  // reverse reads consume the (ascending) rank list from its end: a last entry past the last occurrence of the base
  // (mod_bam.rs:705-727) would never be consumed — the read is rejected here so that hits always form a suffix of the cursor window
  if (rev && T.n[0] && ranks[T.off[0] + T.n[0] - 1u] >= W.tot) acc.err = true;
  const bool trimmable = read_trimmable(prm, W.L);
  uint32_t contribH = 0, qhead = 0, qcount = 0;
  PairWin win; win.wr0 = h.ref_start; win.pref = pairwin_fetch(h, cigar, 0);   // the first CIGAR window, requested before the read is walked
  SparseStep S; sparse_fetch_seq(S, W, 0);

  while (!acc.err) {
    // ---- producer: a loop of its own — the steps and rank batches that refill the queue touch none of the consumer's state, and as
    // iterations of the one outer loop each of them went through that loop's head with all of it
    while (qcount - qhead < 64u && (S.loaded || W.d0 < W.nd)) {
      // the next 64 ranks at the cursor are requested first: the flag / scan work below hides the load
      const RankBatch b = rank_batch(ranks, T.off[0], T.n[0], T.cur[0], rev);
      if (!S.loaded) sparse_count_step(S, W, pat, odd, flg);
      // (reverse reads: the list's last entry was checked against the total, so every entry is below the first window's end)
      const uint32_t cur0 = T.cur[0];
      const RankTake tk = window_take<true>(b, S.wlo, S.whi, rev, T.cur[0]);
      if (tk.nh) {
        if (qhead) queue_to_front<2>(q_pos, MKP_SQCAP, qhead, qcount);
        const uint32_t pos = sparse_locate(S, W, tk.hit, b.e, flg);
        // read order: forward reads hit on the low lanes with ascending positions, reverse reads on the high lanes with descending ones
        const uint32_t slot = qcount + (uint32_t)__popcll(rev ? (tk.lanes & ~lanemask_le()) : (tk.lanes & lanemask_lt()));
        if (tk.hit) { q_pos[slot] = pos; q_idx[slot] = (rev ? cur0 - 64u : cur0) + lane; }
        wave_lds_sync();
        qcount += tk.nh;
      }
      if (tk.nh < 64u) {   // the window holds no further rank: step done; nothing left in the list: the rest of the read holds no call
        W.cum += S.cntT; W.d0 += 512; S.loaded = false;
        if (!list_left_over(rev, T.cur[0], T.n[0])) W.d0 = W.nd;
      }
    }
    if (qcount == qhead) break;
#ifdef MKP_DEBUG
    if (prm.debug_skip & 16u) { qhead += min(64u, qcount - qhead); acc.any_surviving = true; continue; }   // ablation: producer only
#endif
    // The descriptor words the per-call code branches on are made opaque here, once per batch: left visible as loop invariants, every
    // uniform compare derived from them (which code a slot holds, how many codes a tag lists, ...) was hoisted out of the loop as a 64-bit
    // lane mask, dozens of them, spilled to VGPR lanes and read back with two v_readlane each inside the loop — VALU instructions in a
    // VALU-bound kernel; derived in place they are a few scalar instructions that live for a handful of cycles.
    GroupCalls<NT> Gb = G;
    asm volatile("" : "+s"(Gb.g.misc), "+s"(Gb.g.slots), "+s"(Gb.g.cids), "+s"(Gb.kcodes), "+s"(Gb.SH_all), "+s"(Gb.setmask_all));
#pragma unroll
    for (int t = 0; t < NT; t++) asm volatile("" : "+s"(Gb.tmu[t]), "+s"(Gb.t_nc[t]));
    consume_batch<SAMPLE, false, NT>(prm, bedmask, ml, Gb, T.ml, n_tags, W, trimmable, q_pos, q_j, qhead, qcount, win, h, cigar, out, acc, contribH);
  }
  if (list_left_over(rev, T.cur[0], T.n[0])) acc.err = true;
  // InvalidImplicitMode cannot arise (every tag carries '?'), kept for symmetry with the FAST kernels
  group_epilogue<SAMPLE, NT>(prm, lay, G, contribH, acc);
  read_epilogue(readout, ro_idx, acc, duplex);
}

// pdep4[(mask << 4) | bits]: the low bits of `bits` deposited onto the set bits of a 4-bit mask
__device__ __forceinline__ void init_pdep4(uint8_t* pdep4) {
  const uint32_t m = (threadIdx.x >> 4) & 15u; uint32_t f = threadIdx.x & 15u, o = 0;
  for (uint32_t i = 0; i < 4; i++) if ((m >> i) & 1u) { o |= (f & 1u) << i; f >>= 1; }
  pdep4[threadIdx.x & 255u] = (uint8_t)o;
  __syncthreads();
}
// Reads are split by the host into three lists (read_ids): FAST layouts with one tag, FAST layouts with two tags, and
// everything else; each list has its own kernel so the common `C+m?` / `C+h?;C+m?` reads run with few registers and
// little LDS (more waves per SIMD) while the general decoder keeps its full generality.
template <bool SAMPLE, int NT> __device__ __forceinline__ void decode_fast_entry(DECODE_PARAMS(const MkpRunParams&)) {
  __shared__ uint32_t lds_queue[4][(1 + NT) * MKP_QCAP];
  __shared__ __attribute__((aligned(16))) uint32_t lds_layouts[4][MKP_LAYOUT_DWORDS];
  __shared__ uint32_t lds_ord[4][NT * MKP_ORD_WORDS];
  __shared__ uint8_t pdep4[256];
  init_pdep4(pdep4);
  decode_read_fast<SAMPLE, NT>(DECODE_PASS, &lds_layouts[0][0], &lds_ord[0][0], pdep4, &lds_queue[0][0]);
}
template <bool SAMPLE, int NT> __device__ __forceinline__ void decode_sparse_entry(DECODE_PARAMS(const MkpRunParams&)) {
  __shared__ uint32_t lds_queue[4][2 * MKP_SQCAP];
  __shared__ __attribute__((aligned(16))) uint32_t lds_layouts[4][MKP_LAYOUT_DWORDS];
  __shared__ __attribute__((aligned(16))) uint32_t lds_flags[4][512];
  decode_read_sparse<SAMPLE, NT>(DECODE_PASS, &lds_layouts[0][0], &lds_queue[0][0], &lds_flags[0][0]);
}
template <bool SAMPLE> __device__ __forceinline__ void decode_general_entry(DECODE_PARAMS(const MkpRunParams&)) {
  __shared__ __attribute__((aligned(16))) uint32_t lds_layouts[4][MKP_LAYOUT_DWORDS];
  __shared__ uint32_t lds_marks[4 * 7][64];   // per wave 448 dwords: ordinal bitmaps [<=8][18] at 0, 512 u16 slots at 192
  __shared__ uint8_t pdep4[256];
  init_pdep4(pdep4);
  const uint32_t widx = rfl_u(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (widx >= n_reads) return;
  const uint32_t nt = rfl_u(hdrs[read_ids[widx]].n_tags);
#define DECODE_CALL(S, N) decode_read_body<S, N>(DECODE_PASS, &lds_layouts[0][0], lds_marks, pdep4)
  if (nt <= 2) DECODE_CALL(SAMPLE, 2); else if (nt <= 4) DECODE_CALL(SAMPLE, 4); else DECODE_CALL(SAMPLE, MKP_MAX_TAGS);
}
extern "C" __global__ void __launch_bounds__(256) mkp_decode_reads(DECODE_PARAMS(MkpRunParams)) { decode_general_entry<false>(DECODE_PASS); }
extern "C" __global__ void __launch_bounds__(256) mkp_decode_fast1(DECODE_PARAMS(MkpRunParams)) { decode_fast_entry<false, 1>(DECODE_PASS); }
extern "C" __global__ void __launch_bounds__(256) mkp_decode_fast2(DECODE_PARAMS(MkpRunParams)) { decode_fast_entry<false, 2>(DECODE_PASS); }
// Waves per SIMD of the SPARSE event decoders.  Left alone the compiler took 77 / 85 VGPRs and 106 SGPRs = six / five waves; seven
// (72 VGPRs, <= 96 SGPRs: the scalar file admits seven, MI355X_MICROARCH.md "Residency") gave C2 decode 0.509 -> 0.481 ms, hemi 2.40 -> 2.28,
// and eight spilled (0.57 / 2.60).  Since the producer runs as a loop of its own and the consumer's descriptor words are opaque (both
// in decode_read_sparse) the kernels need 59 / 60 VGPRs (55 / 61 with the consumer folded into the shared helpers), and EIGHT waves (<= 64 VGPRs, <= 80 SGPRs) win: C2 decode 0.428 -> 0.405 ms, hemi
// decode 1.955 -> 1.859 (0.452 / 2.03 before both changes).  A/B on one box, tools/dbg/ab.sh.
#ifndef MKP_SPARSE_WAVES
#define MKP_SPARSE_WAVES 8
#endif
#define MKP_SPARSE_LB __launch_bounds__(256, MKP_SPARSE_WAVES)
extern "C" __global__ void MKP_SPARSE_LB mkp_decode_sparse1(DECODE_PARAMS(MkpRunParams)) { decode_sparse_entry<false, 1>(DECODE_PASS); }
extern "C" __global__ void MKP_SPARSE_LB mkp_decode_sparse2(DECODE_PARAMS(MkpRunParams)) { decode_sparse_entry<false, 2>(DECODE_PASS); }
// the same walks in threshold-sampling mode (reads_sampler / thresholds.rs:121-159): separate kernels so profiles keep the two apart
extern "C" __global__ void __launch_bounds__(256) mkp_sample_reads(DECODE_PARAMS(MkpRunParams)) { decode_general_entry<true>(DECODE_PASS); }
extern "C" __global__ void __launch_bounds__(256) mkp_sample_fast1(DECODE_PARAMS(MkpRunParams)) { decode_fast_entry<true, 1>(DECODE_PASS); }
extern "C" __global__ void __launch_bounds__(256) mkp_sample_fast2(DECODE_PARAMS(MkpRunParams)) { decode_fast_entry<true, 2>(DECODE_PASS); }
extern "C" __global__ void __launch_bounds__(256) mkp_sample_sparse1(DECODE_PARAMS(MkpRunParams)) { decode_sparse_entry<true, 1>(DECODE_PASS); }
extern "C" __global__ void __launch_bounds__(256) mkp_sample_sparse2(DECODE_PARAMS(MkpRunParams)) { decode_sparse_entry<true, 2>(DECODE_PASS); }

// ----------------------------------------------------------------------------------------------
// The accumulate kernels of the event pipeline: one 1024-thread workgroup per tile, two per CU (8 waves per SIMD).  The tile's tallies
// live in dynamic LDS, laid out as the host planner sized it (MKP_PILEUP_LDS_WORDS): tallies, hemi's slot map, per-wave scratch.  Waves
// draw the tile's candidate reads from an LDS ticket; after a barrier the rows are produced straight from LDS (mkp_dev_rows.hpp) and
// mkp_scan_tiles / mkp_gather_rows put the tiles' row runs in genome order.  Two bodies, dense and hemi; mkp_dev_tiles.hpp holds the
// little they share.  (Focus runs — --cpg / --motif / --include-bed — are the slot pipeline's, mkp_slots.hip.)

#define PILEUP_PARAMS const MkpReadHdr* __restrict__ hdrs, const uint32_t* __restrict__ cigar, const uint8_t* __restrict__ seqs, \
                 const MkpEvent* __restrict__ events, const MkpReadOut* __restrict__ readout, const MkpTile* __restrict__ tiles, uint32_t n_tiles, \
                 const MkpRunParams* __restrict__ prmp, \
                 uint32_t* __restrict__ rows_base /* 11 SoA arrays of row_capacity entries */, uint32_t* __restrict__ row_cursor, uint32_t* __restrict__ tile_row_off, uint32_t* __restrict__ tile_row_cnt, \
                 const uint2* __restrict__ chunk_pfx, uint32_t* __restrict__ dev_err
#define PILEUP_PASS hdrs, cigar, seqs, events, readout, tiles, n_tiles, prmp, rows_base, row_cursor, tile_row_off, tile_row_cnt, chunk_pfx, dev_err

// Dense tiles (runs without focus positions): every position of the tile's halo'd range [T0h, T1h) owns a tally column, column = p - T0h.
// Tallies are [row][column] u32 with the '+' strand tally in the low and the '-' strand tally in the high 16 bits; rows = the strand
// tally's counters followed by the observed-code slots; consecutive columns sit on consecutive banks.  WIDE (_wide kernels: the host picks
// them for a shard whose deepest column may hold more than 65 535 records) gives every row one u32 plane per strand instead, row r strand
// s at plane 2r + s, at twice the LDS per column.  Per read:
//   * observed codes: +1 / -1 at the columns bounding the read's span (and around ref-skips) — an interval-OR as a difference array;
//   * the read's call events inside the tile: one LDS atomic on the call's counter and -1 on NoCall(read base);
//   * depth walk (htslib pileup columns, pileup/mod.rs:783-939): per 64-op CIGAR window the reference-consuming ops that cover at
//     least one column are compacted through LDS and their first columns marked in the wave's bitmap; deletions are +1 / -1 on a
//     difference array; then one lane per column, 64 columns per step: op index = ballot over the compacted starts + mbcnt of the
//     aligned 64-bit bitmap window, one ds_bpermute fetches the op's packed (query offset, kind), one byte load fetches the base, the
//     1 KB table in LDS maps (strand, query parity, SEQ byte) to the NoCall row, one LDS atomic.
// After a barrier the difference arrays are prefix-summed in place and emit_dense_rows produces the rows of FeatureVector::decode.
// KEYED (--partition-tag): key_arg's low 16 bits = the key this launch tallies, high 16 bits = index of the key pass.
constexpr int DENSE_UNROLL = 4;   // 64-column steps of the depth walk in flight together

template <bool KEYED, bool WIDE>
__device__ __forceinline__ void dense_tiles_body(PILEUP_PARAMS, uint32_t key_arg) {
  const uint32_t key_filter = KEYED ? (key_arg & 0xffffu) : 0u, key_run = KEYED ? (key_arg >> 16) : 0u;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t next_read;
  __shared__ uint32_t wave_tot[PILEUP_WAVES];
  __shared__ uint32_t row_base, row_total;
  __shared__ StreamProg rowprog;   // the row program of the emission (mkp_dev_rows.hpp)
  __shared__ uint8_t rowlut[2][2][256];
  __shared__ __attribute__((aligned(16))) uint32_t prm_lds[(sizeof(MkpRunParams) + 3) / 4];
  tile_prologue(prmp, &rowlut[0][0][0], prm_lds);
  __syncthreads();
  const MkpRunParams& prm = *reinterpret_cast<const MkpRunParams*>(prm_lds);
  const uint32_t S = prm.slot_cap;
#ifdef MKP_DEBUG
  const uint32_t dbg = prm.debug_skip;   // ablation runs (env MKP_DEBUG_SKIP): 1 no depth walk, 2 no events, 4 no row emission
#else
  constexpr uint32_t dbg = 0;
#endif
  constexpr uint32_t NP = WIDE ? 2u : 1u;   // planes per row
  const uint32_t n_counters = prm.n_counters, n_oslots = prm.n_slots;
  const uint32_t tal_words = (n_counters + n_oslots) * S * NP;
  uint32_t* __restrict__ tal = lds;                    // [n_counters + n_oslots][S], packed (WIDE: [n_counters + n_oslots][2][S])
  uint32_t* __restrict__ obs = lds + n_counters * S * NP;   // its tail: the observed-code difference arrays
  const int lane = lane_id();
  const uint32_t wave = rfl_u(threadIdx.x >> 6);
  // per-wave scratch behind the tallies: op-start bitmap over the tile's columns + CIGAR compaction buffer
  const uint32_t bm_words = MKP_PILEUP_BM_WORDS(S), wave_words = MKP_PILEUP_WAVE_WORDS(S, 0u);
  uint32_t* __restrict__ bm = lds + tal_words + wave * wave_words;
  uint2* __restrict__ comp = reinterpret_cast<uint2*>(bm + bm_words);
  const uint32_t TS4 = S * 4u;
  const uint32_t tix = xcd_tile_index(n_tiles);
  const MkpTile tl = tiles[tix];
  const int32_t T0h = tl.r0 - MKP_HALO, T1h = tl.r1 + MKP_HALO;
  const uint32_t n_tslots = (uint32_t)(T1h - T0h);   // tally columns in use
  for (uint32_t k = threadIdx.x; k < tal_words + PILEUP_WAVES * wave_words; k += PILEUP_THREADS) lds[k] = 0;
  if (threadIdx.x == 0) next_read = tl.first;
  __syncthreads();

  const uint32_t rid_end = tl.last;
  TileRead nx;
  draw_read(&next_read, rid_end, hdrs, readout, nx);
  for (;;) {
    if (nx.rid >= rid_end) break;
    const MkpReadHdr h = nx.h; const MkpReadOut ro = nx.ro;
    draw_read(&next_read, rid_end, hdrs, readout, nx);
    if (h.ref_end <= T0h || h.ref_start >= T1h) continue;
    if (KEYED && (h.flags >> MKP_RF_KEY_SHIFT) != key_filter) continue;   // --partition-tag: one pass per key
    const uint32_t rs_a = (uint32_t)(max(h.ref_start, T0h) - T0h), rs_b = (uint32_t)(min(h.ref_end, T1h) - T0h);   // the read's columns
    const uint32_t aln = (h.flags & MKP_RF_REVERSE) ? 1u : 0u;
    const uint8_t* __restrict__ seq = seqs + h.seq_off;
    const CigarStart cs = skip_chunks_before(h, chunk_pfx, T0h);
    uint32_t q_run = cs.q_run; int32_t r_run = cs.r_run;
    // the first chunk's CIGAR words are requested now, ahead of the event work; every later chunk is requested one chunk ahead
    uint32_t w_next = (cs.c_first + (uint32_t)lane < h.n_cigar) ? cigar[h.cigar_off + cs.c_first + lane] : 5u;
    // observed mod codes: +1 over the read's span (add_mod_codes_for_record, pileup/mod.rs:831-835); lane = tally strand
    if (ro.ok && lane < 2) {
      uint32_t m = lane ? ro.obs[1] : ro.obs[0];
      while (m) {
        const uint32_t sl = (uint32_t)__ffs((int)m) - 1u; m &= m - 1u;
        obs_diff<WIDE>(obs, S, sl, (uint32_t)lane, rs_a, rs_b, n_tslots, false);
      }
    }
    if (ro.ok && ro.n_events && !(dbg & 2u))
      for_tile_events(events + h.event_off, ro.n_events, h.ref_start >= T0h, T0h, T1h, [&](uint32_t, const MkpEvent& e) {
        const uint32_t i = (uint32_t)((int32_t)e.pos - T0h);
        if (WIDE) {   // [8] tally strand of the call, [11] of the read's base
          atomicAdd(&tal[(2u * (e.info & 0xffu) + ((e.info >> 8) & 1u)) * S + i], 1u);
          if (e.info & (1u << 12)) atomicAdd(&tal[(2u * (MKP_C_NC + ((e.info >> 9) & 3u)) + ((e.info >> 11) & 1u)) * S + i], 0u - 1u);
        } else {
          atomicAdd(&tal[(e.info & 0xffu) * S + i], (e.info & 0x100u) ? 0x10000u : 1u);
          if (e.info & (1u << 12))  // the base is a call, not a NoCall (pileup/mod.rs:889-938)
            atomicAdd(&tal[(MKP_C_NC + ((e.info >> 9) & 3u)) * S + i], 0u - ((e.info & 0x800u) ? 0x10000u : 1u));
        }
      });
    // depth walk: htslib pileup columns (match -> base, D -> delete, N -> ref-skip).  One lane per column;
    // the op covering a column = (ops whose first column is at or before it) - 1, counted with the wave's op-start bitmap.
    const uint32_t inc = WIDE ? 1u : (aln ? 0x10000u : 1u);   // this alignment strand's half of the packed tallies
    // WIDE: this alignment strand's plane of a row (byte offset) and the distance between two rows' planes
    const uint32_t aln_plane = WIDE ? aln * S * 4u : 0u, row_bytes = WIDE ? S * 8u : S * 4u;
    const uint8_t* __restrict__ lut = &rowlut[0][0][0];
    const uint32_t aln2 = aln << 1;
    const uint32_t lanebase = lds_addr(tal) + 4u * (uint32_t)lane;   // LDS byte address of (row 0, column `lane`)
    const uint32_t qbase = (uint32_t)(0 - h.ref_start) - (1u << 26);   // query index = position + qbase + packed offset
    const uint32_t last_byte = (h.l_seq - 1u) >> 1;
    if (!(dbg & 1u))
    for (uint32_t c0 = cs.c_first; c0 < h.n_cigar; c0 += 64) {
      if (r_run >= T1h) break;
      const uint32_t w = w_next;
      if (c0 + 64u < h.n_cigar) w_next = (c0 + 64u + (uint32_t)lane < h.n_cigar) ? cigar[h.cigar_off + c0 + 64u + lane] : 5u;
      const uint32_t op = w & 15u, len = w >> 4;
      const uint32_t qlen = op_consumes_query(op) ? len : 0u, rlen = op_consumes_ref(op) ? len : 0u;
      const uint32_t qe = wave_incl_scan(qlen), re = wave_incl_scan(rlen);
      const uint32_t qs = q_run + qe - qlen;
      const int32_t rs = r_run + (int32_t)(re - rlen);
      const uint32_t Qtot = (uint32_t)__builtin_amdgcn_readlane((int)qe, 63), Rtot = (uint32_t)__builtin_amdgcn_readlane((int)re, 63);
      const int32_t c_lo = max(r_run, T0h), c_hi = min(r_run + (int32_t)Rtot, T1h);
      if (c_lo < c_hi) {
        // the op's columns inside the tile: [sa, sb)
        const uint32_t sa = (uint32_t)(min(max(rs, c_lo), c_hi) - T0h), sb = (uint32_t)(min(max(rs + (int32_t)rlen, c_lo), c_hi) - T0h);
        const bool covers = rlen > 0 && sa < sb;
        if (op == 3 && ro.ok && covers) {  // ref-skip: the read is not in these columns (alignment.is_refskip())
          for (uint32_t s = 0; s < 2; s++) {
            uint32_t m = ro.obs[s];
            while (m) {
              const uint32_t sl = (uint32_t)__ffs((int)m) - 1u; m &= m - 1u;
              obs_diff<WIDE>(obs, S, sl, s, sa, sb, n_tslots, true);
            }
          }
        }
        if (op == 2 && covers) {  // deletion columns (alignment.is_del()): +1/-1 on the strand's DEL row, summed after the barrier
          const uint32_t del_row = WIDE ? (2u * MKP_C_DEL + aln) * S : MKP_C_DEL * S;
          atomicAdd(&tal[del_row + sa], inc);
          if (sb < n_tslots) atomicAdd(&tal[del_row + sb], 0u - inc);
        }
        const uint32_t S_lo = (uint32_t)(c_lo - T0h), S_hi = (uint32_t)(c_hi - T0h);   // the chunk's columns
        // compact the window's column-covering ops to the low lanes: {first column, packed(query offset, kind)}
        const unsigned long long refbal = __ballot(covers);
        const uint32_t nref = (uint32_t)__popcll(refbal);
        const uint32_t ci = (uint32_t)__popcll(refbal & lanemask_lt());
        const uint32_t kind = op_is_match(op) ? 0u : (op == 2 ? 1u : 2u);
        // q = (pos - ref_start) + D; kind sits where it ORs into the row
        const uint32_t pk = ((uint32_t)((int32_t)qs - (rs - h.ref_start) + (1 << 26)) << 5) | (kind << 3);
        if (covers) comp[ci] = make_uint2(sa, pk);
        wave_lds_sync();
        const uint2 cc = comp[lane];
        const bool cvalid = (uint32_t)lane < nref;
        const uint32_t c_sa = cc.x; const uint32_t c_pk = cc.y;
        const uint32_t c_key = cvalid ? c_sa : 0x7fffffffu;
        const uint32_t e_lo = lds_addr(tal) + 4u * S_lo, e_span = 4u * (S_hi - S_lo);
        const bool mark = cvalid && c_sa > S_lo;
        const uint32_t mrel = c_sa - 1u;   // bit m set <=> an op's first column is m+1: "starts at or before column c" = bits strictly below c
        if (mark) atomicOr(&bm[mrel >> 5], 1u << (mrel & 31u));
        wave_lds_sync();
        // 64 columns per step, aligned so a step reads one aligned 64-bit window of the bitmap;
        // DENSE_UNROLL steps are issued together (bitmap read -> bpermute -> SEQ byte load) before any tally update.
        // ops started at or before the first column of window kk: a ballot over the compacted starts (no LDS dependency)
        const uint32_t k0 = S_lo >> 6, k1 = (S_hi - 1u) >> 6;
        // Only the first and the last group of a chunk hold out-of-range lanes or repeated (clamped) windows; the groups in
        // between run a version without the clamps and the range check.
        auto group = [&](uint32_t kb, auto edge_c) {
          constexpr bool EDGE = decltype(edge_c)::value;
          constexpr int U = DENSE_UNROLL;
          uint32_t pkv[U], byte[U], qq[U], idx[U], kk[U]; uint2 Wd[U];
          // stage by stage across the U windows, so the LDS reads, the bpermutes and the global loads of the group overlap
#pragma unroll
          for (int j = 0; j < U; j++) kk[j] = EDGE ? min(kb + (uint32_t)j, k1) : kb + (uint32_t)j;
#pragma unroll
          for (int j = 0; j < U; j++) Wd[j] = *reinterpret_cast<const uint2*>(bm + 2u * kk[j]);
#pragma unroll
          for (int j = 0; j < U; j++) {
            const uint32_t wstart = 64u * kk[j];
            idx[j] = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(c_key <= (EDGE ? max(S_lo, wstart) : wstart))) - 1u;
          }
#pragma unroll
          for (int j = 0; j < U; j++)
            pkv[j] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((idx[j] + __builtin_amdgcn_mbcnt_hi(Wd[j].y,
                __builtin_amdgcn_mbcnt_lo(Wd[j].x, 0u))) << 2), (int)c_pk);
#pragma unroll
          for (int j = 0; j < U; j++) {
            qq[j] = (uint32_t)(T0h + (int32_t)(64u * kk[j]) + lane) + qbase + (pkv[j] >> 5);
            byte[j] = seq[min(qq[j] >> 1, last_byte)];   // lanes on D/N ops or outside the span read a clamped (ignored) byte
          }
#pragma unroll
          for (int j = 0; j < U; j++) {
            const uint32_t t = (qq[j] & 1u) | aln2;
            const uint32_t rowt = (uint32_t)lut[(t << 8) | byte[j]] | (pkv[j] & 0x18u);   // >= 8: not ACGT, or the lane sits on a D/N op
            const uint32_t la = lanebase + 256u * kk[j];
            bool ok = rowt < 8u;
            if (EDGE) ok = ok && (la - e_lo) < e_span && kb + (uint32_t)j <= k1;
            if (ok) lds_add(la + (WIDE ? __umul24(rowt, row_bytes) + aln_plane : __umul24(rowt, TS4)), inc);
          }
        };
        for (uint32_t kb = k0; kb <= k1; kb += DENSE_UNROLL) {
          if (kb == k0 || kb + DENSE_UNROLL > k1) group(kb, std::true_type{}); else group(kb, std::false_type{});
        }
        if (mark) bm[mrel >> 5] = 0;
      }
      q_run += Qtot; r_run += (int32_t)Rtot;
    }
  }
  __syncthreads();
  // difference arrays -> counts, one wave per array: the DEL row (WIDE: its two planes), then the observed-code rows, which are
  // contiguous behind `obs` in either layout
  for (uint32_t a = wave; a < NP * (n_oslots + 1u); a += PILEUP_WAVES)
    prefix_sum_in_place(a < NP ? tal + (NP * MKP_C_DEL + a) * S : obs + (a - NP) * S, n_tslots);
  __syncthreads();
  // rows of the tile straight from LDS.  One tile per workgroup: nothing of the accumulate phase is live here and nothing of this phase
  // is live there, so neither raises the other's register count.  The row map takes the per-wave scratch (dead behind the barrier).
  if (!(dbg & 4u))
    emit_dense_rows<WIDE>(tal, S, n_counters, n_tslots, T0h, tl, KEYED ? key_run * n_tiles + tix : tix, key_filter, prm, rowprog,
        lds + tal_words, min(8192u, PILEUP_WAVES * wave_words), rows_base, row_cursor, tile_row_off, tile_row_cnt, dev_err, wave_tot,
        &row_base, &row_total);
}

// pileup-hemi tiles (duplex.rs:241-339): only the '+' motif positions of [T0h, T1h) own a tally column (SlotMap, built from the run's
// slot bitmap; the host caps a tile at one column per thread), so a tile covers ~50x more reference for the same LDS.  Counters are plain
// u32 [counter][column] (MKP_H_*), every update a +1: a read's '+' tally call at a column and its '-' tally call at the partner
// position form one pattern count.  The depth walk is driven by the columns, not by the ops: 128 CIGAR ops per window (two per lane).
// Phase 1 leaves each column of the read's visit its packed (query index, kind) in the wave's scratch; phase 2 fetches the bases with
// several SEQ loads in flight — they do not sit in the CIGAR dependency chain.  Then emit_hemi_rows.
__device__ __forceinline__ void hemi_tiles_body(PILEUP_PARAMS, const uint32_t* __restrict__ slotbm) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t next_read;
  __shared__ uint32_t wave_tot[PILEUP_WAVES];
  __shared__ uint32_t row_base, scan_carry;   // scan_carry: running column count while the slot map is built, then the tile's row total
  __shared__ uint8_t rowlut[2][2][256];
  __shared__ __attribute__((aligned(16))) uint32_t prm_lds[(sizeof(MkpRunParams) + 3) / 4];
  tile_prologue(prmp, &rowlut[0][0][0], prm_lds);
  __syncthreads();
  const MkpRunParams& prm = *reinterpret_cast<const MkpRunParams*>(prm_lds);
  const uint32_t S = prm.slot_cap, W = prm.focus_words;
#ifdef MKP_DEBUG
  const uint32_t dbg = prm.debug_skip;   // ablation runs (env MKP_DEBUG_SKIP): 1 no depth walk, 4 no row emission, 8 no SEQ phase
#else
  constexpr uint32_t dbg = 0;
#endif
  const uint32_t tal_words = prm.hemi_counters * S;
  uint32_t* __restrict__ tal = lds;                       // [hemi_counters][S]
  uint32_t* __restrict__ fbm = lds + tal_words;           // slot map: bitmap words [W], running popcount [W], column -> position [S]
  uint32_t* __restrict__ fpfx = fbm + W;
  int32_t* __restrict__ fpos = reinterpret_cast<int32_t*>(fpfx + W);
  const int lane = lane_id();
  const uint32_t wave = rfl_u(threadIdx.x >> 6);
  // per-wave scratch behind that: per column of the current read's visit, (query index << 2) | kind; kind 3 = no base
  const uint32_t wave_words = MKP_PILEUP_WAVE_WORDS(S, W), scratch0 = tal_words + 2u * W + S;
  uint32_t* __restrict__ qk = lds + scratch0 + wave * wave_words;
  const uint32_t TS4 = S * 4u;
  const uint32_t tix = xcd_tile_index(n_tiles);
  const MkpTile tl = tiles[tix];
  const int32_t T0h = tl.r0 - MKP_HALO, T1h = tl.r1 + MKP_HALO;
  for (uint32_t k = threadIdx.x; k < tal_words; k += PILEUP_THREADS) lds[k] = 0;
  for (uint32_t k = threadIdx.x; k < PILEUP_WAVES * wave_words; k += PILEUP_THREADS) lds[scratch0 + k] = 3u;
  if (threadIdx.x == 0) { next_read = tl.first; scan_carry = 0; }
  // the tile's slice of the slot bitmap: words masked to [T0h, T1h), their running popcount, and the column -> position list
  SlotMap sm; sm.bm = fbm; sm.pfx = fpfx; sm.fpos = fpos;
  {
    const uint32_t g0 = (uint32_t)(T0h - (prm.win_start - MKP_SLOTBM_MARGIN)), sh = g0 & 31u, nbits = (uint32_t)(T1h - T0h);
    const uint32_t nw = (sh + nbits + 31u) >> 5;
    sm.lbase = T0h - (int32_t)sh;
    __syncthreads();   // scan_carry = 0 visible
    for (uint32_t k0 = 0; k0 < nw + 1u; k0 += PILEUP_THREADS) {
      const uint32_t k = k0 + threadIdx.x;
      uint32_t w = 0;
      if (k < nw) {
        w = slotbm[(g0 >> 5) + k];
        if (k == 0) w &= ~((1u << sh) - 1u);
        const uint32_t endb = sh + nbits - 32u * k;   // bits of this word below the range end
        if (endb < 32u) w &= (1u << endb) - 1u;
      }
      const uint32_t cnt = (uint32_t)__popc(w), inc = wave_incl_scan(cnt);
      if (lane == 63) wave_tot[wave] = inc;
      __syncthreads();
      uint32_t woff = scan_carry;
      for (uint32_t w2 = 0; w2 < wave; w2++) woff += wave_tot[w2];
      const uint32_t excl = woff + inc - cnt;
      if (k <= nw) { fbm[k] = w; fpfx[k] = excl; }
      for (uint32_t ww = w, j = 0; ww; ww &= ww - 1u, j++) fpos[excl + j] = sm.lbase + (int32_t)(32u * k) + (__ffs((int)ww) - 1);
      __syncthreads();
      if (threadIdx.x == PILEUP_THREADS - 1) scan_carry = woff + inc;
    }
    __syncthreads();
  }
  const uint32_t n_tslots = scan_carry;   // tally columns in use
  __syncthreads();

  const uint32_t rid_end = tl.last;
  TileRead nx;
  draw_read(&next_read, rid_end, hdrs, readout, nx);
  if (n_tslots) for (;;) {
    if (nx.rid >= rid_end) break;
    const MkpReadHdr h = nx.h; const MkpReadOut ro = nx.ro;
    draw_read(&next_read, rid_end, hdrs, readout, nx);
    if (h.ref_end <= T0h || h.ref_start >= T1h) continue;
    // the read's columns in this tile; a read that covers none leaves nothing here
    const uint32_t rs_a = sm.rank(max(h.ref_start, T0h)), rs_b = sm.rank(min(h.ref_end, T1h));
    if (rs_a == rs_b) continue;
    const uint8_t* __restrict__ seq = seqs + h.seq_off;
    const CigarStart cs = skip_chunks_before(h, chunk_pfx, T0h);
    uint32_t q_run = cs.q_run; int32_t r_run = cs.r_run;
    // the first window's CIGAR words are requested now, ahead of the event work; every later window is requested one window ahead
    auto load2 = [&](uint32_t c) { uint2 r; const uint32_t i = c + 2u * (uint32_t)lane; r.x = i < h.n_cigar ? cigar[h.cigar_off + i] : 5u;
      r.y = i + 1u < h.n_cigar ? cigar[h.cigar_off + i + 1u] : 5u; return r; };
    uint2 w2_next = load2(cs.c_first);
    // get_duplex_mod_call (read_cache.rs:422-462) over the read's call events inside the tile: a '+' tally call at a column = the
    // positive-strand half; its partner is the read's '-' tally call on the same primary base at position + hemi_off (a few events
    // away).  Both present -> one pattern (or Filtered) count and the NoCall the walk below adds for this base is taken back;
    // otherwise the base stays a NoCall.  A record whose tags failed carries, instead of calls, the one NoCall per interval the
    // reference's cache leaves for it (mkp_hemi_failed_reads).
    if (ro.n_events) {
      const MkpEvent* __restrict__ ev = events + h.event_off;
      const int32_t hoff = prm.hemi_off;
      // threshold base of the call (read_cache.rs:147-150)
      auto pb_of = [](uint32_t info) { const uint32_t b = (info >> 9) & 3u; return (((info >> 11) ^ (info >> 8)) & 1u) ? 3u - b : b; };
      for_tile_events(ev, ro.n_events, h.ref_start >= T0h, T0h, T1h, [&](uint32_t k, const MkpEvent& e) {
        if (!sm.is_slot((int32_t)e.pos)) return;
        const uint32_t i = sm.rank((int32_t)e.pos);
        if (!ro.ok) { atomicAdd(&tal[(e.info & 0xffu) * S + i], 1u); return; }
        if (e.info & 0x100u) return;
        const uint32_t pbA = pb_of(e.info);
        const int32_t q = (int32_t)e.pos + hoff;
        uint32_t binfo = 0xffffffffu;
        if (hoff >= 0) for (uint32_t j = k + 1u; j < ro.n_events; j++) {
          const MkpEvent f = ev[j];
          if ((int32_t)f.pos > q) break;
          if ((int32_t)f.pos == q && (f.info & 0x100u) && pb_of(f.info) == pbA) { binfo = f.info; break; }
        }
        if (hoff <= 0 && binfo == 0xffffffffu) for (uint32_t j = k; j-- > 0u;) {
          const MkpEvent f = ev[j];
          if ((int32_t)f.pos < q) break;
          if ((int32_t)f.pos == q && (f.info & 0x100u) && pb_of(f.info) == pbA) { binfo = f.info; break; }
        }
        if (binfo != 0xffffffffu && q >= 0) {
          const uint32_t elA = prm.hemi_el[e.info & 0xffu], elB = prm.hemi_el[binfo & 0xffu];
          const uint32_t cid = (elA == 0xffu || elB == 0xffu) ? (uint32_t)MKP_H_FAIL + pbA
              : (uint32_t)prm.hemi_pat_base[pbA] + elA * prm.hemi_nel[pbA] + elB;
          atomicAdd(&tal[cid * S + i], 1u);
          atomicAdd(&tal[(MKP_H_NC + pbA) * S + i], 0u - 1u);
        }
      });
    }
    const uint8_t* __restrict__ lut = &rowlut[0][0][0];   // (the primary base is the SEQ base as stored, whatever the strand: duplex.rs:308-313)
    const uint32_t qbase = (uint32_t)(0 - h.ref_start) - (1u << 26);   // query index = position + qbase + packed offset
    const uint32_t last_byte = (h.l_seq - 1u) >> 1;
    // phase 1.  A window's columns [S_lo, S_hi) are enumerated 64 at a time (lane = column, position from the slot map's list); the lane
    // holding a position's op is the number of lanes whose inclusive reference end is at or before it (6 ds_bpermute steps over the
    // prefix sums the window has anyway), three more bpermutes bring that lane's split point and the packed (query offset, kind) of
    // its two ops.  No per-op rank queries, no compaction, no op-start bitmap.
    if (!(dbg & 1u))
    for (uint32_t c0 = cs.c_first; c0 < h.n_cigar; c0 += 128) {
      if (r_run >= T1h) break;
      const uint2 w2 = w2_next;
      if (c0 + 128u < h.n_cigar) w2_next = load2(c0 + 128u);
      const uint32_t op0 = w2.x & 15u, len0 = w2.x >> 4, op1 = w2.y & 15u, len1 = w2.y >> 4;
      const uint32_t ql0 = op_consumes_query(op0) ? len0 : 0u, rl0 = op_consumes_ref(op0) ? len0 : 0u;
      const uint32_t ql1 = op_consumes_query(op1) ? len1 : 0u, rl1 = op_consumes_ref(op1) ? len1 : 0u;
      const uint32_t qe = wave_incl_scan(ql0 + ql1), re = wave_incl_scan(rl0 + rl1);
      const uint32_t Qtot = (uint32_t)__builtin_amdgcn_readlane((int)qe, 63), Rtot = (uint32_t)__builtin_amdgcn_readlane((int)re, 63);
      const int32_t c_lo = max(r_run, T0h), c_hi = min(r_run + (int32_t)Rtot, T1h);
      if (c_lo < c_hi) {
        const uint32_t S_lo = sm.rank(c_lo), S_hi = sm.rank(c_hi);
        if (S_lo < S_hi) {
          const uint32_t qs0 = q_run + qe - (ql0 + ql1), qs1 = qs0 + ql0;
          const uint32_t mid = re - rl1;                                     // window-relative reference offset where the lane's second op starts
          const int32_t rs0 = r_run + (int32_t)(re - (rl0 + rl1)), rs1 = r_run + (int32_t)mid;
          const uint32_t kind0 = op_is_match(op0) ? 0u : (op0 == 2 ? 1u : 2u), kind1 = op_is_match(op1) ? 0u : (op1 == 2 ? 1u : 2u);
          const uint32_t pk0 = ((uint32_t)((int32_t)qs0 - (rs0 - h.ref_start) + (1 << 26)) << 5) | (kind0 << 3);  // q = (pos - ref_start) + D
          const uint32_t pk1 = ((uint32_t)((int32_t)qs1 - (rs1 - h.ref_start) + (1 << 26)) << 5) | (kind1 << 3);
          for (uint32_t s0 = S_lo; s0 < S_hi; s0 += 64) {
            const uint32_t c = s0 + (uint32_t)lane;
            const bool valid = c < S_hi;
            const int32_t p = valid ? fpos[c] : c_lo;
            const uint32_t rel = (uint32_t)(p - r_run);
            const int ol = find_op(re, rel) & 63;
            const uint32_t o_mid = (uint32_t)__shfl((int)mid, ol, 64), o_pk0 = (uint32_t)__shfl((int)pk0, ol, 64),
                o_pk1 = (uint32_t)__shfl((int)pk1, ol, 64);
            const uint32_t my_pk = rel < o_mid ? o_pk0 : o_pk1;
            const uint32_t qq = (uint32_t)p + qbase + (my_pk >> 5);
            if (valid) qk[c - rs_a] = (qq << 2) | ((my_pk >> 3) & 3u);
          }
        }
      }
      q_run += Qtot; r_run += (int32_t)Rtot;
    }
    if (!(dbg & 9u)) {
      // phase 2: bases of the read's columns [rs_a, rs_b), 4 x 64 columns per round with their SEQ loads in flight together
      // (columns the CIGAR phase did not reach — a read whose CIGAR ends early — keep kind 3 = nothing)
      wave_lds_sync();
      const uint32_t nsl = rs_b - rs_a;
      for (uint32_t g0 = 0; g0 < nsl; g0 += 256) {
        uint32_t v[4], byte[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { const uint32_t i = g0 + 64u * j + (uint32_t)lane; v[j] = i < nsl ? qk[i] : 3u; }
#pragma unroll
        for (int j = 0; j < 4; j++) byte[j] = seq[min(v[j] >> 3, last_byte)];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t i = g0 + 64u * j + (uint32_t)lane, kind = v[j] & 3u;
          const uint32_t rowt = (uint32_t)lut[(((v[j] >> 2) & 1u) << 8) | byte[j]];   // NoCall row of the base; >= 8: not ACGT
          const uint32_t a0 = lds_addr(tal) + 4u * (rs_a + i);
          // a failed record gives no feature (its one NoCall came in as an event)
          if (kind == 0u && rowt < 8u && ro.ok) lds_add(a0 + __umul24(rowt, TS4), 1u);
          if (kind == 1u) lds_add(a0 + __umul24((uint32_t)MKP_H_DEL, TS4), 1u);   // alignment.is_del(): counted directly
          if (i < nsl) qk[i] = 3u;   // left clean for the wave's next read
        }
      }
      wave_lds_sync();
    }
  }
  // (no difference arrays here, so no prefix-sum phase: deletions are counted per column above, and a duplex column has no
  // observed-code rows)
  __syncthreads();
  if (!(dbg & 4u))
    emit_hemi_rows(tal, sm, n_tslots, tl, tix, prm, rows_base, row_cursor, tile_row_off, tile_row_cnt, dev_err, wave_tot, &row_base, &scan_carry);
}

// every position owns a tally column (no focus positions)
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_tiles(PILEUP_PARAMS, uint32_t key_arg /* unused */) {
  dense_tiles_body<false, false>(PILEUP_PASS, key_arg); }
// --partition-tag: the same kernel tallying only the reads of one partition key per launch
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_tiles_keyed(PILEUP_PARAMS, uint32_t key_arg) {
  dense_tiles_body<true, false>(PILEUP_PASS, key_arg); }
// shards whose deepest column may hold more than 65 535 records: u32 tallies per strand
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_tiles_wide(PILEUP_PARAMS, uint32_t key_arg /* unused */) {
  dense_tiles_body<false, true>(PILEUP_PASS, key_arg); }
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_tiles_keyed_wide(PILEUP_PARAMS, uint32_t key_arg) {
  dense_tiles_body<true, true>(PILEUP_PASS, key_arg); }
// pileup-hemi
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_tiles_hemi(PILEUP_PARAMS, const uint32_t* __restrict__ slotbm) {
  hemi_tiles_body(PILEUP_PASS, slotbm); }

// Duplex reads decoded one group per wave (decode_read_sparse): interleave the two position-sorted event lists of a read into the
// front of its slice and combine the two summaries.  The record fails if either group failed (add_record returns at the first
// error, read_cache.rs:111-211) and counts as "no modified base information" if neither group added anything.
extern "C" __global__ void __launch_bounds__(256)
mkp_merge_duplex(const MkpReadHdr* __restrict__ hdrs, const uint32_t* __restrict__ read_ids, uint32_t n, const MkpTagRef* __restrict__ tagref,
    const MkpLayout* __restrict__ layouts,
                 MkpEvent* __restrict__ events, MkpReadOut* __restrict__ readout, uint32_t roff) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t widx = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (widx >= n) return;
  const uint32_t rid_raw = (uint32_t)__builtin_amdgcn_readfirstlane((int)read_ids[widx]);
  if (rid_raw >> 31) return;   // the listing of the second group
  const uint32_t rid = rid_raw;
  const MkpReadHdr h = hdrs[rid];
  const uint32_t n_first = layouts[h.layout].pad;
  const uint32_t capA = tagref[h.tag_off].n, capB = tagref[h.tag_off + n_first].n;
  const MkpReadOut a = readout[rid], b = readout[roff + rid];
  MkpReadOut out; out.n_events = 0; out.ok = 0; out.obs[0] = 0; out.obs[1] = 0;
  if (a.ok && b.ok && (a.ok == 1u || b.ok == 1u)) {
    const MkpEvent* __restrict__ eA = events + h.event_off + capA + capB; const MkpEvent* __restrict__ eB = eA + capA;
    MkpEvent* __restrict__ dst = events + h.event_off;
    const uint32_t nA = a.ok == 1u ? a.n_events : 0u, nB = b.ok == 1u ? b.n_events : 0u;
    // An event of the first group goes after the second group's events at lower positions, one of the second group after the first group's
    // events at lower or equal positions.  Both lists are sorted, so the ranks of 64 consecutive events of one list lie in a short window of
    // the other: the window's positions are taken 64 at a time, one per lane, and every lane finds its rank with six cross-lane steps
    // (round 5: a bisection over global memory per event — eight dependent loads; 2 x 0.33 ms per pass of the hemi workload).
    auto place = [&](const MkpEvent* __restrict__ X, uint32_t nX, const MkpEvent* __restrict__ Y, uint32_t nY, uint32_t le) {
      uint32_t y0 = 0;   // (uniform) every Y entry before y0 ranks below every X event still to come
      for (uint32_t i0 = 0; i0 < nX; i0 += 64u) {
        const uint32_t i = i0 + lane; const bool valid = i < nX;
        MkpEvent e; e.pos = 0xfffffffeu; e.info = 0; if (valid) e = X[i];
        const uint32_t key = e.pos + le;   // "<= pos" as "< pos + 1"
        uint32_t rank = y0;
        for (uint32_t yw = y0;; yw += 64u) {
          const uint32_t yv = yw + lane < nY ? Y[yw + lane].pos : 0xffffffffu;
          uint32_t c = (uint32_t)find_sorted(yv, key);         // entries of this window below the key (find_sorted stops at 63: the last lane's own
          if (c == 63u && (uint32_t)__shfl((int)yv, 63, 64) < key) c = 64u;   // entry is looked at here)
          const bool more = valid && rank == yw && c == 64u;   // the whole window ranks below this lane's key: the next one may too
          if (valid && rank == yw) rank += c;
          if (!__any(more) || yw + 64u >= nY) break;
        }
        if (valid) dst[i + rank] = e;
        y0 = (uint32_t)__builtin_amdgcn_readlane((int)rank, (int)(min(nX - i0, 64u) - 1u));
      }
    };
    place(eA, nA, eB, nB, 0u);
    place(eB, nB, eA, nA, 1u);
    out.ok = 1; out.n_events = nA + nB;
    out.obs[0] = (a.ok == 1u ? a.obs[0] : 0u) | (b.ok == 1u ? b.obs[0] : 0u);
      out.obs[1] = (a.ok == 1u ? a.obs[1] : 0u) | (b.ok == 1u ? b.obs[1] : 0u);
  }
  if (lane == 0) readout[rid] = out;
}

// pileup-hemi, records whose tags failed (readout.ok == 0): DuplexReadCache::get_duplex_mod_call (read_cache.rs:422-462) finds such a
// record in no map the first time it is asked about it, fails to add it, and answers NoCall(primary base) for that one position;
// from then on the record is in the skip set and yields no feature.  The cache lives for one interval (process_region_duplex,
// duplex.rs:241-339), so the record leaves one NoCall per interval it crosses: at its first '+' motif position there that it
// covers with an A/C/G/T base (not a deletion or ref-skip).  One thread per record writes those as events into the record's own
// (unused) event slice, where mkp_pileup_tiles_hemi picks them up.  iv_start = ascending starts of the shard's intervals.
extern "C" __global__ void __launch_bounds__(256)
mkp_hemi_failed_reads(const MkpReadHdr* __restrict__ hdrs, const uint32_t* __restrict__ cigar, const uint8_t* __restrict__ seqs,
    MkpEvent* __restrict__ events,
                      MkpReadOut* __restrict__ readout, uint32_t n_reads, const uint32_t* __restrict__ slotbm, const uint32_t* __restrict__ iv_start,
                          uint32_t n_iv,
                      int32_t win_start, int32_t win_end, uint32_t* __restrict__ dev_err) {
  const uint32_t rid = blockIdx.x * 256u + threadIdx.x;
  if (rid >= n_reads) return;
  if (readout[rid].ok) return;
  const MkpReadHdr h = hdrs[rid];
  const uint8_t* __restrict__ seq = seqs + h.seq_off;
  MkpEvent* __restrict__ ev = events + h.event_off;
  auto next_slot = [&](int32_t a, int32_t b) -> int32_t {   // first slot in [a, b), or -1
    uint32_t bit = (uint32_t)(a - (win_start - MKP_SLOTBM_MARGIN));
    const uint32_t end = (uint32_t)(b - (win_start - MKP_SLOTBM_MARGIN));
    uint32_t w = slotbm[bit >> 5] & ~((1u << (bit & 31u)) - 1u);
    for (;;) {
      if (w) { const uint32_t f = (bit & ~31u) + (uint32_t)__ffs((int)w) - 1u; return f < end ? (int32_t)f + (win_start - MKP_SLOTBM_MARGIN) : -1; }
      bit = (bit & ~31u) + 32u;
      if (bit >= end) return -1;
      w = slotbm[bit >> 5];
    }
  };
  uint32_t n = 0, q = 0; bool overflow = false;
  int32_t rp = h.ref_start, served = max(h.ref_start, win_start);   // positions below `served` lie in intervals that have their NoCall
  for (uint32_t c = 0; c < h.n_cigar && rp < win_end && served < win_end; c++) {
    const uint32_t w = cigar[h.cigar_off + c], op = w & 15u, len = w >> 4;
    if (op_is_match(op)) {
      int32_t a = max(rp, served); const int32_t b = min(rp + (int32_t)len, win_end);
      while (a < b) {
        const int32_t p = next_slot(a, b);
        if (p < 0) break;
        const uint32_t qq = q + (uint32_t)(p - rp);
        const int x = qq < h.l_seq ? nib2base(seq_nibble(seq, qq)) : -1;
        if (x < 0) { a = p + 1; continue; }
        if (n < h.event_cap) { ev[n].pos = (uint32_t)p; ev[n].info = (uint32_t)(MKP_H_NC + x); } else overflow = true;
        n++;
        uint32_t lo = 0, hi = n_iv;   // first interval starting after p
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (iv_start[mid] <= (uint32_t)p) lo = mid + 1u; else hi = mid; }
        served = lo < n_iv ? (int32_t)iv_start[lo] : win_end;
        a = served;
      }
    }
    if (op_consumes_query(op)) q += len;
    if (op_consumes_ref(op)) rp += (int32_t)len;
  }
  if (overflow) { atomicOr(dev_err, ERR_EVENT_CAP); n = 0; }
  readout[rid].n_events = n;
}

// ----------------------------------------------------------------------------------------------
// Order the per-tile row runs by tile index.  Block 0 computes the exclusive scan of the
// tile counts (n_tiles is small), then every block copies its tiles' runs.
extern "C" __global__ void __launch_bounds__(1024)
mkp_scan_tiles(const uint32_t* __restrict__ tile_row_cnt, uint32_t n_tiles, uint32_t* __restrict__ tile_dst_off, uint32_t* __restrict__ total_rows) {
  __shared__ uint32_t carry_s;
  __shared__ uint32_t wtot[16];
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < n_tiles; b0 += 1024) {
    const uint32_t k = b0 + threadIdx.x;
    const uint32_t v = k < n_tiles ? tile_row_cnt[k] : 0u;
    const uint32_t inc = wave_incl_scan(v);
    if (lane_id() == 63) wtot[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t woff = 0;
    for (uint32_t w2 = 0; w2 < (threadIdx.x >> 6); w2++) woff += wtot[w2];
    if (k < n_tiles) tile_dst_off[k] = carry_s + woff + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s += woff + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total_rows = carry_s;
}

extern "C" __global__ void __launch_bounds__(256)
mkp_gather_rows(const uint32_t* __restrict__ tile_row_off, const uint32_t* __restrict__ tile_row_cnt, const uint32_t* __restrict__ tile_dst_off,
                uint32_t n_tiles, MkpRowsDev src, MkpRowsDev dst) {
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t n = tile_row_cnt[t], so = tile_row_off[t], d0 = tile_dst_off[t];
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
      dst.pos[d0 + k] = src.pos[so + k]; dst.info[d0 + k] = src.info[so + k]; dst.code[d0 + k] = src.code[so + k];
      dst.n_valid[d0 + k] = src.n_valid[so + k]; dst.n_mod[d0 + k] = src.n_mod[so + k]; dst.n_can[d0 + k] = src.n_can[so + k];
      dst.n_other[d0 + k] = src.n_other[so + k]; dst.n_del[d0 + k] = src.n_del[so + k]; dst.n_fail[d0 + k] = src.n_fail[so + k];
      dst.n_diff[d0 + k] = src.n_diff[so + k]; dst.n_nocall[d0 + k] = src.n_nocall[so + k];
    }
  }
}

// ----------------------------------------------------------------------------------------------
// Threshold estimation (thresholds.rs:121-159) without shipping the sample to the host: the argmax probabilities the
// mkp_sample_* kernels wrote stay in HBM.  The f32 bit pattern of a probability is its sort key (positive floats order like
// unsigned integers); patterns are below 2^30, so the canonical base of a value rides in the top two bits.
//   mkp_sample_accumulate  for the reads the host's sampling schedule took: append {base, pattern} keys to the resident sample
//                          and count the top 16 bits of every pattern per base (level-0 histogram: LDS-privatised window of the
//                          patterns probabilities actually have, global atomics for the rest)
//   mkp_sample_hist1       level-1 histogram: the low 16 bits of the keys of one base whose top 16 bits equal `prefix`
// Two levels give the exact order statistics percentile_linear_interp needs (a 2 x 16 bit radix select); both histograms are
// plain integer arrays that add across GPUs (the path's one collective).
#define MKP_HIST_LO 0x3800u     // top-16 patterns [0x3800, 0x4000) = values in [2^-15, 2) are counted in LDS
#define MKP_HIST_LDS 2048u
extern "C" __global__ void __launch_bounds__(256)
mkp_sample_accumulate(const MkpReadHdr* __restrict__ hdrs, const MkpReadOut* __restrict__ readout, const uint8_t* __restrict__ take, uint32_t n_reads,
                      const float* __restrict__ vals, const MkpEvent* __restrict__ events, uint32_t* __restrict__ store, unsigned long long store_cap,
                      unsigned long long* __restrict__ store_cursor, uint32_t* __restrict__ hist0, uint32_t* __restrict__ dev_err) {
  __shared__ uint32_t lh[4][MKP_HIST_LDS];
  for (uint32_t k = threadIdx.x; k < 4u * MKP_HIST_LDS; k += 256) (&lh[0][0])[k] = 0;
  __syncthreads();
  const int lane = lane_id();
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
  for (uint32_t r = wave; r < n_reads; r += n_waves) {
    if (!take[r]) continue;
    const MkpReadOut ro = readout[r];
    if (!ro.ok || !ro.n_events) continue;
    const uint32_t e0 = hdrs[r].event_off;
    for (uint32_t k0 = 0; k0 < ro.n_events; k0 += 64) {
      const uint32_t k = k0 + (uint32_t)lane;
      const bool v = k < ro.n_events;
      uint32_t key = 0;
      if (v) { const uint32_t bits = __float_as_uint(vals[e0 + k]), base = events[e0 + k].info & 3u; key = (base << 30) | (bits & 0x3fffffffu);
               const uint32_t top = (bits >> 16) & 0x3fffu;
               if (top - MKP_HIST_LO < MKP_HIST_LDS) atomicAdd(&lh[base][top - MKP_HIST_LO], 1u); else atomicAdd(&hist0[base * 65536u + top], 1u); }
      const unsigned long long b = __ballot(v);
      unsigned long long at = 0;
      if (lane == 0) at = atomicAdd(store_cursor, (unsigned long long)__popcll(b));
      at = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(at >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)at);
      const unsigned long long idx = at + (unsigned long long)__popcll(b & lanemask_lt());
      if (v) { if (idx < store_cap) store[idx] = key; else atomicOr(dev_err, ERR_EVENT_CAP); }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < 4u * MKP_HIST_LDS; k += 256) { const uint32_t c = (&lh[0][0])[k];
    if (c) atomicAdd(&hist0[(k / MKP_HIST_LDS) * 65536u + MKP_HIST_LO + (k % MKP_HIST_LDS)], c);
    }
}

extern "C" __global__ void __launch_bounds__(256)
mkp_sample_hist1(const uint32_t* __restrict__ store, unsigned long long n, uint32_t base, uint32_t prefix, uint32_t* __restrict__ hist1) {
  const uint32_t want = (base << 14) | (prefix & 0x3fffu);   // key >> 16
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256u) {
    const uint32_t key = store[i];
    if ((key >> 16) == want) atomicAdd(&hist1[key & 0xffffu], 1u);
  }
}

// `modkit summary`: counts of the sampled calls of the reads the schedule took.  table[base][0 pass | 1 filtered][class] (class as in
// summary_info; filtered calls are counted under their argmax class), reads_with[base] = taken reads with a call on that base,
// reads_with[4] = taken reads with any call, reads_with[5] = OR of the reads' observed-code slot masks.
extern "C" __global__ void __launch_bounds__(256)
mkp_summary_accumulate(const MkpReadHdr* __restrict__ hdrs, const MkpReadOut* __restrict__ readout, const uint8_t* __restrict__ take,
    uint32_t n_reads,
                       const MkpEvent* __restrict__ events, unsigned long long* __restrict__ table /*[4][2][16]*/,
                           unsigned long long* __restrict__ reads_with /*[6]*/) {
  __shared__ uint32_t lt[128];
  __shared__ uint32_t lr[6];
  for (uint32_t k = threadIdx.x; k < 128; k += 256) lt[k] = 0;
  if (threadIdx.x < 6) lr[threadIdx.x] = 0;
  __syncthreads();
  const int lane = lane_id();
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
  for (uint32_t r = wave; r < n_reads; r += n_waves) {
    if (!take[r]) continue;
    const MkpReadOut ro = readout[r];
    if (!ro.ok || !ro.n_events) continue;
    const uint32_t e0 = hdrs[r].event_off;
    uint32_t bases = 0;
    for (uint32_t k0 = 0; k0 < ro.n_events; k0 += 64) {
      const uint32_t k = k0 + (uint32_t)lane;
      if (k < ro.n_events) {
        const uint32_t info = events[e0 + k].info, tb = info & 3u, thr = (info >> 4) & 15u, arg = (info >> 8) & 15u;
        atomicAdd(&lt[tb * 32u + (thr ? thr : 16u + arg)], 1u);
        bases |= 1u << tb;
      }
    }
    bases = wave_or(bases);
    if (lane == 0) { for (uint32_t b = 0; b < 4; b++) if (bases & (1u << b)) atomicAdd(&lr[b], 1u); atomicAdd(&lr[4], 1u);
      atomicOr(&lr[5], ro.obs[0] | ro.obs[1]); }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < 128; k += 256) if (lt[k]) atomicAdd(&table[k], (unsigned long long)lt[k]);
  if (threadIdx.x < 5 && lr[threadIdx.x]) atomicAdd(&reads_with[threadIdx.x], (unsigned long long)lr[threadIdx.x]);
  if (threadIdx.x == 5 && lr[5]) atomicOr(&reads_with[5], (unsigned long long)lr[5]);
}
// host-side launchers of the sampling kernels (declared in mkp_launch.h)
extern "C" hipError_t mkp_launch_summary_accumulate(hipStream_t st, const MkpShardArrays& sh, const uint8_t* take, uint32_t n_reads,
    unsigned long long* table, unsigned long long* reads_with) {
  if (!n_reads) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((n_reads + 3u) / 4u, 1024u);
  hipLaunchKernelGGL(mkp_summary_accumulate, dim3(grid), dim3(256), 0, st, sh.hdr, sh.readout, take, n_reads, sh.events, table, reads_with);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_sample_accumulate(hipStream_t st, const MkpShardArrays& sh, const uint8_t* take, uint32_t n_reads,
    const float* vals, uint32_t* store, unsigned long long store_cap, unsigned long long* store_cursor, uint32_t* hist0, uint32_t* dev_err) {
  if (!n_reads) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((n_reads + 3u) / 4u, 1024u);
  hipLaunchKernelGGL(mkp_sample_accumulate, dim3(grid), dim3(256), 0, st, sh.hdr, sh.readout, take, n_reads, vals, sh.events, store, store_cap,
      store_cursor, hist0, dev_err);
  return hipGetLastError();
}
extern "C" hipError_t mkp_launch_sample_hist1(hipStream_t st, const uint32_t* store, unsigned long long n, uint32_t base, uint32_t prefix,
    uint32_t* hist1) {
  if (!n) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<unsigned long long>((n + 255u) / 256u, 4096ull);
  hipLaunchKernelGGL(mkp_sample_hist1, dim3(grid), dim3(256), 0, st, store, n, base, prefix, hist1);
  return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------
// host-side launchers (declared in mkp_launch.h)
// read_ids = [SPARSE one tag | SPARSE two tags | FAST one tag | FAST two tags | all other reads], n_class = the five list lengths
extern "C" hipError_t mkp_launch_decode(hipStream_t st, const MkpShardArrays& sh, const uint32_t* read_ids, const uint32_t* n_class /* [7] */,
    const MkpRunParams* prm, uint32_t* dev_err, const uint8_t* bedmask, float* sample_vals) {
  const MkpReadHdr* hdrs = sh.hdr; const uint32_t* cigar = sh.cigar; const uint8_t* seqs = sh.seq; const MkpTagRef* tagref = sh.tagref;
  const uint32_t* ranks = sh.ranks; const uint8_t* ml = sh.ml; const MkpLayout* layouts = sh.layouts; MkpEvent* events = sh.events;
  MkpReadOut* readout = sh.readout;
  const uint32_t waves_per_block = 4;
  const uint32_t* ids = read_ids;
  for (int cls = 0; cls < 7; cls++) {
    const uint32_t n = n_class[cls];
    if (n) {
      dim3 grid((n + waves_per_block - 1) / waves_per_block), block(64 * waves_per_block);
      if (cls >= 5) {   // duplex reads, listed once per group (never in sampling mode): SPARSE decode per group, then the merge
        if (prm->sample_mode) return hipErrorInvalidValue;
        if (cls == 5) hipLaunchKernelGGL(mkp_decode_sparse1, grid, block, 0, st, hdrs, n, cigar, seqs, tagref, ranks, ml, layouts, *prm, events,
            readout, dev_err, bedmask, sample_vals, ids);
        else hipLaunchKernelGGL(mkp_decode_sparse2, grid, block, 0, st, hdrs, n, cigar, seqs, tagref, ranks, ml, layouts, *prm, events, readout,
            dev_err, bedmask, sample_vals, ids);
        hipLaunchKernelGGL(mkp_merge_duplex, grid, block, 0, st, hdrs, ids, n, tagref, layouts, events, readout, prm->readout_b_off);
        ids += n;
        continue;
      }
#define MKP_DECODE_LAUNCH(K) hipLaunchKernelGGL(K, grid, block, 0, st, hdrs, n, cigar, seqs, tagref, ranks, ml, layouts, *prm, events, readout, dev_err, bedmask, sample_vals, ids)
      if (prm->sample_mode) { if (cls == 0) MKP_DECODE_LAUNCH(mkp_sample_sparse1); else if (cls == 1) MKP_DECODE_LAUNCH(mkp_sample_sparse2);
        else if (cls == 2) MKP_DECODE_LAUNCH(mkp_sample_fast1);
        else if (cls == 3) MKP_DECODE_LAUNCH(mkp_sample_fast2);
        else MKP_DECODE_LAUNCH(mkp_sample_reads);
        }
      else { if (cls == 0) MKP_DECODE_LAUNCH(mkp_decode_sparse1); else if (cls == 1) MKP_DECODE_LAUNCH(mkp_decode_sparse2);
        else if (cls == 2) MKP_DECODE_LAUNCH(mkp_decode_fast1);
        else if (cls == 3) MKP_DECODE_LAUNCH(mkp_decode_fast2);
        else MKP_DECODE_LAUNCH(mkp_decode_reads);
        }
    }
    ids += n;
  }
  return hipGetLastError();
}

// per device: both accumulate kernels may use the whole per-workgroup LDS budget the host planned for
extern "C" hipError_t mkp_pileup_set_lds(uint32_t accum_bytes) {
  for (const void* k : {(const void*)mkp_pileup_tiles, (const void*)mkp_pileup_tiles_keyed, (const void*)mkp_pileup_tiles_hemi,
                        (const void*)mkp_pileup_tiles_wide, (const void*)mkp_pileup_tiles_keyed_wide}) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)accum_bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// hemi: pileup-hemi (slotbm = the run's slot bitmap); otherwise a run without focus positions (slotbm unused)
extern "C" hipError_t mkp_launch_pileup(hipStream_t st, uint32_t lds_bytes, bool hemi, const MkpShardArrays& sh, const MkpTile* tiles,
    uint32_t n_tiles, const MkpRunParams* prm_dev, const uint32_t* slotbm, const MkpRowsDev* rows, uint32_t* row_cursor, uint32_t* tile_row_off,
    uint32_t* tile_row_cnt, uint32_t* dev_err, uint32_t key_filter, uint32_t key_slot, bool wide) {
  if (!n_tiles) return hipSuccess;
  const bool keyed = key_filter != MKP_NO_KEY_FILTER;
  const uint32_t key_arg = keyed ? ((key_filter & 0xffffu) | (key_slot << 16)) : 0u;
  const uint32_t grid = n_tiles;   // one workgroup per tile
  // ONE build of each accumulate kernel: what a one-shot shard pass launches is what a re-launch on the resident shard launches
#define MKP_PILEUP_LAUNCH(K, LAST) hipLaunchKernelGGL(K, dim3(grid), dim3(PILEUP_THREADS), lds_bytes, st, sh.hdr, sh.cigar, sh.seq, sh.events, sh.readout, \
                       tiles, n_tiles, prm_dev, rows->pos, row_cursor, tile_row_off, tile_row_cnt, reinterpret_cast<const uint2*>(sh.chunk_pfx), dev_err, LAST)
  if (hemi) MKP_PILEUP_LAUNCH(mkp_pileup_tiles_hemi, slotbm);
  else if (wide) { if (keyed) MKP_PILEUP_LAUNCH(mkp_pileup_tiles_keyed_wide, key_arg); else MKP_PILEUP_LAUNCH(mkp_pileup_tiles_wide, key_arg); }   // u32 tallies
  else { if (keyed) MKP_PILEUP_LAUNCH(mkp_pileup_tiles_keyed, key_arg); else MKP_PILEUP_LAUNCH(mkp_pileup_tiles, key_arg); }
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_hemi_failed(hipStream_t st, const MkpShardArrays& sh, uint32_t n_reads, const uint32_t* slotbm,
    const uint32_t* iv_start, uint32_t n_iv, int32_t win_start, int32_t win_end, uint32_t* dev_err) {
  if (!n_reads) return hipSuccess;
  hipLaunchKernelGGL(mkp_hemi_failed_reads, dim3((n_reads + 255u) / 256u), dim3(256), 0, st, sh.hdr, sh.cigar, sh.seq, sh.events, sh.readout,
      n_reads, slotbm, iv_start, n_iv, win_start, win_end, dev_err);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_gather(hipStream_t st, const uint32_t* tile_row_off, const uint32_t* tile_row_cnt, uint32_t* tile_dst_off,
                                        uint32_t n_tiles, uint32_t* total_rows, const MkpRowsDev* src, const MkpRowsDev* dst) {
  hipLaunchKernelGGL(mkp_scan_tiles, dim3(1), dim3(1024), 0, st, tile_row_cnt, n_tiles, tile_dst_off, total_rows);
  if (n_tiles) {
    uint32_t grid = n_tiles < 2048u ? n_tiles : 2048u;
    hipLaunchKernelGGL(mkp_gather_rows, dim3(grid), dim3(256), 0, st, tile_row_off, tile_row_cnt, tile_dst_off, n_tiles, *src, *dst);
  }
  return hipGetLastError();
}
