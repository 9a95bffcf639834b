// gfx950 (CDNA4, wave64) kernels of the SLOT PIPELINE: the modkit-pileup hot path for runs with focus positions (--cpg, --motif,
// --include-bed — FocusPositions::{Motif, MotifCombineStrands, Regions}, interval_chunks.rs:32-59).  A "slot" is a focus position;
// the host numbers the window's slots in genome order (slot_pos[g] = position of global slot g) and gives every read the slot
// range [gs0, gs0 + n_sl) of its reference span.  One device pass:
//
//   mkp_call_plane        once per resident shard: per fused read and 32 stored bases one 8-byte entry in each of TWO planes — the call
//                         plane: one bit per base "a listed call sits here" and the number of listed calls before the 32 bases; the base
//                         plane: the bases' 2-bit codes (the SEQ and the rank list resolved against each other: nothing of it depends on
//                         the pass)
//   mkp_decode_slots      one wave per read, reads whose MM tags form one explicit-mode ('?') group with one shared delta list
//                         (`C+m?`, `C+hm?`, `C+h?;C+m?` as basecallers write them), no edge filter.  The walk is driven by the
//                         read's SLOTS, not by its calls, 64 slots per step: CIGAR (256-op register window, reference -> query; read from
//                         the 16-bit array, 8 bytes per lane and window, unless an op of the read is longer than 4 095 bases), the
//                         whether a call is listed there and as which call (one 8-byte gather from the call plane), the base only where
//                         none is listed (one dword of the base plane: a listed call's feature replaces the coverage feature, so most
//                         slots never touch the base plane; a read without calls gathers its base entries instead and never touches
//                         the call plane; the SEQ byte only for a read with a base that is not A/C/G/T),
//                         ML -> f32 probabilities -> MultipleThresholdModCaller::call, and ONE FEATURE BYTE per slot goes to the
//                         read's run of the feature stream — for the slots of the read's own strand only where it feeds one tally
//                         strand and the shard's rules tell the strands apart (the slot-entry lists, mkp_plan.hpp: under --cpg half of a
//                         read's slots; the other bytes stay MKP_FB_BLANK from the prefill).
//                         Calls on non-focus positions are never located (their rows would be
//                         dropped, pileup/mod.rs:570-604); CIGAR is read once per pass, the plane only under the slots.
//   mkp_cover_reads       every other read (implicit-mode / multi-group / duplex / `N` tags / failed tags, or any read when an edge
//                         filter is set): the decode kernels of mkp_kernels.hip leave position-sorted call events; this kernel walks
//                         the read's slots (coverage features) and merges the events into the stream.
//   mkp_pileup_stream     accumulate + emit: one workgroup per tile of <= 1024 slots; the tile's reads' feature bytes are a
//                         position-implicit stream (byte k of a read = global slot gs0 + k): four bytes per lane, one LDS atomic per
//                         feature on 16-bit-packed strand tallies; observed codes as difference arrays; rows straight from LDS
//                         (emit_stream_rows, mkp_dev_rows.hpp), the runs in genome order through a look-back.  This is the
//                         packed-event-stream histogram of BASELINE.json's north_star.
//   mkp_dup_restore / mkp_dup_events / mkp_dup_apply   records that share a read name inside one interval
// and, in front of them, the one CIGAR window walker (CigarWin, cigwin_*: reference -> query) of the decoder, mkp_cover_reads and
// mkp_dup_events; behind them the host-side launchers.
//
// Semantics follow /root/reference/src (cited inline).  f32 arithmetic is the reference's (contraction off, IEEE division).
#include <cstdlib>

#include "mkp_base_pack.hpp"
#include "mkp_cigar_pack.hpp"
#include "mkp_dev_common.hpp"
#include "mkp_dev_rows.hpp"
#include "mkp_launch.h"

// per-wave LDS of mkp_decode_slots: the read's caller constants per code (integer pass threshold, offset and stride of its ML bytes,
// counter of Modified(code)) — uniform, but the kernel is short of scalar registers: every lane reads them back as vectors once per slot batch
struct SlotLds { int32_t ck_thr[4]; uint32_t ck_off[4]; uint32_t ck_str[4]; uint32_t ck_cid[4]; };

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t feat(uint32_t cid, uint32_t tally) { return cid | (tally << 5); }

// loads as `uniform base + 32-bit byte offset`: the address is one VALU instruction (global saddr form), not 64-bit arithmetic
template <class T> __device__ __forceinline__ T ldo(const void* __restrict__ base, uint32_t byte_off) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off); }
// per op code (MIDNSHP=X): bit 0 consumes query, bit 1 consumes reference, bits 2-3 kind
#define MKP_CIGAR_LUT 0x888888833889a693ull

// The CIGAR as the slot walks see it (the decoder, mkp_cover_reads, mkp_dup_events): 256 ops per window (four per lane), reference ->
// query.  re = inclusive reference end of the lane's four ops (window-relative), m1..m3 = where its second..fourth op start, pk[j] =
// ((query start - (reference start - ref_start)) << 2) | kind (0 match: M = X, 1 deletion, 2 ref-skip / nothing) of op j.
// The decoder is VALU-issue bound and this mapping was 42 % of its vector instructions, hence: the window's running values live in scalar
// registers (read back through readfirstlane after every update: left to itself the compiler carries them as vectors and advances them
// with v_cndmask), "nothing loaded yet" is a window of no reference bases in front of op 0 — no flag, no conditional advance — and a step
// maps its lanes in a pass of straight-line code, with the loop only behind it for the steps that straddle windows.
struct CigarWin { uint32_t c0, q_run, Rtot, Qtot; int32_t r_run; uint32_t re, m1, m2, m3, pk[4]; uint4 pref; };
// A lane's four ops come from the read's 16-bit CIGAR (mkp_cigar_pack.hpp) as ONE 8-byte load — the read starts on a multiple of four
// entries, and so does every lane; a read with an op that does not fit 16 bits (MKP_RF_CIGW), and every read of the kernels that read the
// BAM words (`wide`, uniform over the wave), takes the 16-byte load of its 32-bit words instead.  cg = the read's first op in the array it is
// read from.  The address is clamped to the read's last quad (inside its own room) / last op (the buffer has slack behind it).  The branch
// is at the load only, and nothing touches the loaded registers before the window is opened (the request stays one window ahead):
// cigar_quad_ops then widens the 16-bit ops back to BAM words — ops past the end read as 0H.
typedef const __attribute__((address_space(1))) char* MkpCigarPtr;   // (a pointer into global memory, whichever of the two arrays it came from)
__device__ __forceinline__ uint4 cigar_quad_load(MkpCigarPtr cg, bool wide, uint32_t n_cigar, uint32_t c) {
  typedef uint32_t U2 __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) U2* P2;
  const uint32_t k = c + 4u * (uint32_t)lane_id();
  // the first eight bytes of either form are one load (the clamp and the entry size are scalars); the BAM words' other eight follow
  const uint32_t off = min(k, wide ? n_cigar - 1u : (n_cigar - 1u) & ~3u) << (wide ? 2u : 1u);
  const U2 lo = *reinterpret_cast<P2>(cg + off);
  uint4 r; r.x = lo.x; r.y = lo.y;   // (.z, .w are read of a wide read only)
  if (wide) { const U2 hi = *reinterpret_cast<P2>(cg + off + 8u); r.z = hi.x; r.w = hi.y; }
  return r;
}
__device__ __forceinline__ uint4 cigar_quad_ops(uint4 r, bool wide, uint32_t n_cigar, uint32_t c) {
  const uint32_t k = c + 4u * (uint32_t)lane_id();
  if (!wide) r = make_uint4(mkp_cigar16_unpack(r.x), mkp_cigar16_unpack(r.x >> 16), mkp_cigar16_unpack(r.y), mkp_cigar16_unpack(r.y >> 16));
  if (__any(k + 4u > n_cigar)) { if (k >= n_cigar) r.x = 5u; if (k + 1u >= n_cigar) r.y = 5u; if (k + 2u >= n_cigar) r.z = 5u;
    if (k + 3u >= n_cigar) r.w = 5u;
    }
  return r;
}
__device__ __forceinline__ void cigwin_init(CigarWin& w, MkpCigarPtr cg, bool wide, uint32_t n_cigar, int32_t ref_start) {
  w.c0 = 0u - 256u; w.q_run = 0; w.r_run = ref_start; w.Rtot = 0; w.Qtot = 0; w.re = w.m1 = w.m2 = w.m3 = 0;
    w.pk[0] = w.pk[1] = w.pk[2] = w.pk[3] = 0;
  w.pref = cigar_quad_load(cg, wide, n_cigar, 0);
}
// the next 256 ops; false behind the last op
__device__ __forceinline__ bool cigwin_next(CigarWin& w, MkpCigarPtr cg, bool wide, uint32_t n_cigar, int32_t ref_start) {
  w.c0 = rfl(w.c0 + 256u); w.q_run = rfl(w.q_run + w.Qtot); w.r_run = (int32_t)rfl((uint32_t)w.r_run + w.Rtot);
  if (w.c0 >= n_cigar) { w.Rtot = 0; w.Qtot = 0; return false; }
  const uint4 v = cigar_quad_ops(w.pref, wide, n_cigar, w.c0);
  w.pref = cigar_quad_load(cg, wide, n_cigar, w.c0 + 256u);   // requested one window ahead
  const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
  uint32_t ql[4], rl[4], kind[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t f = (uint32_t)(MKP_CIGAR_LUT >> ((wd[j] & 15u) << 2)), len = wd[j] >> 4;
    ql[j] = len & (0u - (f & 1u)); rl[j] = len & (0u - ((f >> 1) & 1u)); kind[j] = (f >> 2) & 3u;
  }
  const uint32_t qsum = ql[0] + ql[1] + ql[2] + ql[3], rsum = rl[0] + rl[1] + rl[2] + rl[3];
  uint32_t qe;
  if (!__any((v.x | v.y | v.z | v.w) >= (128u << 4))) {   // ops shorter than 128: both running sums fit 16 bits, one scan serves both
    const uint32_t sc = wave_incl_scan(qsum | (rsum << 16));
    qe = sc & 0xffffu; w.re = sc >> 16;
  } else { qe = wave_incl_scan(qsum); w.re = wave_incl_scan(rsum); }
  w.Qtot = (uint32_t)__builtin_amdgcn_readlane((int)qe, 63); w.Rtot = (uint32_t)__builtin_amdgcn_readlane((int)w.re, 63);
  // d = query offset - (reference offset - ref_start) of the lane's op, carried op to op; rs = window-relative reference offset
  uint32_t rs = w.re - rsum;
  uint32_t d = (w.q_run - (uint32_t)(w.r_run - ref_start)) + (qe - qsum) - rs;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    w.pk[j] = (d << 2) | kind[j];
    d += ql[j] - rl[j]; rs += rl[j];
    if (j == 0) w.m1 = rs; else if (j == 1) w.m2 = rs; else if (j == 2) w.m3 = rs;
  }
  return true;
}
// one pass over the lanes whose position lies in the loaded window
__device__ __forceinline__ void cigwin_pass(const CigarWin& w, int32_t ref_start, bool& pending, int32_t p, uint32_t& kind, uint32_t& q) {
  const uint32_t rel0 = (uint32_t)(p - w.r_run);
  const bool inw = pending && rel0 < w.Rtot;
  if (!__any(inw)) return;
  const uint32_t rel = inw ? rel0 : 0u;
  uint32_t probe = 31u << 2;
#pragma unroll
  for (int hstep = 16; hstep >= 1; hstep >>= 1) {
    const uint32_t vv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)probe, (int)w.re);
    probe = vv <= rel ? probe + 4u * (uint32_t)hstep : probe - 4u * (uint32_t)hstep;
  }
  { const uint32_t vv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)probe, (int)w.re); probe = vv <= rel ? probe + 4u : probe; }
  const int oa = (int)(probe & 255u);
  const uint32_t o_m1 = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)w.m1), o_m2 = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)w.m2),
      o_m3 = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)w.m3);
  const uint32_t o0 = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)w.pk[0]), o1 = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)w.pk[1]);
  const uint32_t o2 = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)w.pk[2]), o3 = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)w.pk[3]);
  const uint32_t pk = rel < o_m1 ? o0 : rel < o_m2 ? o1 : rel < o_m3 ? o2 : o3;
  if (inw) { kind = pk & 3u; q = (uint32_t)((p - ref_start) + ((int32_t)pk >> 2)); pending = false; }
}
__device__ __forceinline__ void cigwin_map(CigarWin& w, MkpCigarPtr cg, bool wide, uint32_t n_cigar, int32_t ref_start, bool valid, int32_t p,
    uint32_t* kind_out, uint32_t* q_out) {
  bool pending = valid; uint32_t kind = 2u, q = 0u;
  cigwin_pass(w, ref_start, pending, p, kind, q);
  while (__any(pending)) {
    if (!cigwin_next(w, cg, wide, n_cigar, ref_start)) break;   // (cannot happen for positions inside the span)
    cigwin_pass(w, ref_start, pending, p, kind, q);
  }
  *kind_out = kind; *q_out = q;
}

// coverage feature of a slot: NoCall(base) on the alignment strand (the base complemented on '-': get_forward_read_base,
// pileup/mod.rs:612-624), Delete, nothing on a ref-skip, and no feature for a base that is not A/C/G/T (864-874)
__device__ __forceinline__ uint32_t cover_feature(uint32_t kind, uint32_t nib, uint32_t aln) {
  if (kind == 1u) return feat(MKP_C_DEL, aln);
  if (kind != 0u) return MKP_FB_NONE;
  const int sb = nib2base(nib);
  if (sb < 0) return MKP_FB_BLANK;
  return feat((uint32_t)MKP_C_NC + (aln ? 3u - (uint32_t)sb : (uint32_t)sb), aln);
}

// ----------------------------------------------------------------------------------------------------------------------
// mkp_call_plane: the call plane and the base plane of the fused reads (MkpCallEnt, MkpBaseEnt, mkp_device.h), built once when the shard
// becomes resident — what they answer (is a listed call at this stored index, and which one; the base there) depends on the SEQ, the rank
// list, the strand and the tag's fundamental base only, never on the pass.  One wave per work record; every fused read gets its bases, the
// call entries are zero for a read without calls (two 8-byte stores per 32 bases, one into either plane):
//   one walk over the read's words in the order the tag counts its base (a reverse read from its last word, its flag bitmaps bit-reversed),
//   64 plane entries (2 048 bases) per step: the entries' 2-bit base codes (mkp_pack_bases32; a base that is not A/C/G/T sets MKP_RF_SEQN)
//   and, for a read with calls, the words' flag bitmaps (mkp_bases_eq) and their occurrence counts (a wave scan), then the rank list's
//   entries that fall on the step's occurrences, in list order, each placed on its word (a search over the lanes' counts) and its bit (the
//   (o - count)-th flag of the word); the word's listed calls before it in stored order follow from the running count and a wave scan.  A
//   delta list whose last entry is not below the base's occurrence count runs past its last occurrence (mod_bam.rs:705-727): entries are
//   left unplaced, MKP_RF_RUNOVER in the work record.
// seqn_bytes collects what the decoder will read of the SEQN reads' SEQ (one byte per decoded slot, at most the read's bytes): algorithmic bytes.
// Reference: DeltaListConverter::new / to_positions (mod_bam.rs:667-733).
extern "C" __global__ void __launch_bounds__(256) mkp_call_plane(MkpWork* __restrict__ work, uint32_t n_reads, const uint8_t* __restrict__ seqs,
    const uint32_t* __restrict__ ranks, const MkpFusedDesc* __restrict__ fdesc, MkpCallEnt* __restrict__ call_plane, MkpBaseEnt* __restrict__ base_plane,
    unsigned long long* __restrict__ seqn_bytes) {
  __shared__ uint32_t bm_all[4][64];
  const int lane = lane_id();
  const uint32_t wib = rfl(threadIdx.x >> 6);
  const uint32_t widx = rfl(blockIdx.x * (blockDim.x >> 6)) + wib;
  if (widx >= n_reads) return;
  const MkpWork h = work[widx];
  const uint32_t t_n = h.n_calls;
  bool calls = !(h.flags & MKP_RF_BAD) && h.n_tags != 0 && t_n != 0;   // without calls the decoder reads only the bases
  uint32_t flags = h.flags;
  uint32_t* __restrict__ bm = bm_all[wib];
  const bool rev = (h.flags & MKP_RF_REVERSE) != 0;
  const uint32_t L = h.l_seq, nd = (L + 7u) >> 3, nw = MKP_PLANE_WORDS(L);
  const uint8_t* __restrict__ seqb = seqs + h.seq_off;
  const uint32_t* __restrict__ rk = ranks + h.rank_off;
  // the four SEQ dwords of plane word w; dwords at or past the read's end read as 0
  auto word_seq = [&](uint32_t w) {
    const uint32_t d = 4u * w;
    uint4 x = ldo<uint4>(seqb, 4u * min(d, nd - 1u));   // (clamped to the read's last dword: the SEQ buffer has slack behind the last read)
    if (d + 1u >= nd) x.y = 0u; if (d + 2u >= nd) x.z = 0u; if (d + 3u >= nd) x.w = 0u; if (d >= nd) x.x = 0u;
    return x;
  };
  const uint32_t fb = calls ? fdesc[h.layout].misc & 3u : 0u;
  const uint32_t sb = rev ? 3u - fb : fb;   // the stored base the tags count
  // The words are walked in the order the tag counts its base: a forward read from its first word, a reverse read from its last (word
  // w = nw - 1 - k at walk index k, its flag bitmap bit-reversed), so that the rank list is consumed from its start and the walk's running
  // occurrence count IS the rank — no pass that counts the base first.  256 words per chunk, four per lane (k = k0 + 64 j + lane): four
  // 16-byte SEQ loads in flight, packed into the entries' base codes and, for a read with calls, the flag bitmaps taken from the codes.
  uint32_t lo[4], hi[4], f[4];
  bool seqn = false;
  auto word_of = [&](uint32_t k) { return rev ? nw - 1u - k : k; };
  auto load_chunk = [&](uint32_t k0) {
    uint4 x[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t k = k0 + 64u * (uint32_t)j + (uint32_t)lane;
      x[j] = k < nw ? word_seq(word_of(k)) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t k = k0 + 64u * (uint32_t)j + (uint32_t)lane, w = word_of(k);
      uint32_t l = 0u, hh = 0u, fl = 0u;
      if (k0 + 64u * (uint32_t)j < nw && k < nw) {   // (the first test is uniform: a quarter without a word of the read is not packed)
        const uint32_t b0 = 32u * w, nv = b0 >= L ? 0u : min(L - b0, 32u);
        const uint32_t bad = mkp_pack_bases32(x[j].x, x[j].y, x[j].z, x[j].w, nv, &l, &hh);
        seqn = seqn || bad != 0u;
        if (calls) {
          fl = mkp_bases_eq(l, hh, sb) & ~bad & (nv >= 32u ? 0xffffffffu : (1u << nv) - 1u);
          if (rev) fl = __brev(fl);
        }
      }
      lo[j] = l; hi[j] = hh; f[j] = fl;
    }
  };
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  u32x2* __restrict__ pl_call = reinterpret_cast<u32x2*>(call_plane + h.pad);
  u32x2* __restrict__ pl_base = reinterpret_cast<u32x2*>(base_plane + h.pad);
  uint32_t occ = 0, j = 0;   // occurrences before the step, listed calls before the step (both in walk order)
  for (uint32_t k0 = 0; k0 < nw; k0 += 256u) {
    load_chunk(k0);
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {   // 64 words per step
      if (k0 + 64u * (uint32_t)jj >= nw) break;
      const uint32_t k = k0 + 64u * (uint32_t)jj + (uint32_t)lane, w = word_of(k);
      uint32_t lw = 0, before = 0;
      if (calls) {
        const uint32_t fw = f[jj], c = (uint32_t)__popc(fw);
        const uint32_t incl = wave_incl_scan(c), cnt = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t j0 = j;
        bm[lane] = 0u;
        wave_lds_sync();
        for (;;) {
          const uint32_t i = j + (uint32_t)lane;
          const bool valid = i < t_n;
          const uint32_t e = valid ? ldo<uint32_t>(rk, 4u * i) : 0u;
          const uint32_t rel = e - occ;   // (entries below the step were consumed by the steps before)
          const bool hit = valid && rel < cnt;
          const uint32_t rq = hit ? rel : 0u;
          // the word: the number of lanes whose inclusive count is <= rel (six probes)
          uint32_t probe = 31u << 2;
#pragma unroll
          for (int hstep = 16; hstep >= 1; hstep >>= 1) {
            const uint32_t vv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)probe, (int)incl);
            probe = vv <= rq ? probe + 4u * (uint32_t)hstep : probe - 4u * (uint32_t)hstep;
          }
          { const uint32_t vv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)probe, (int)incl); probe = vv <= rq ? probe + 4u : probe; }
          const int oa = (int)(probe & 255u);
          const uint32_t fo = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)fw), io = (uint32_t)__builtin_amdgcn_ds_bpermute(oa, (int)incl);
          // the bit: the n-th flag of the word (halving select)
          uint32_t n = rq - (io - (uint32_t)__popc(fo)), pos = 0;
#pragma unroll
          for (int s = 16; s >= 1; s >>= 1) {
            const uint32_t lo_n = (uint32_t)__popc((fo >> pos) & ((1u << s) - 1u));
            if (n >= lo_n) { n -= lo_n; pos += (uint32_t)s; }
          }
          if (hit) atomicOr(&bm[probe >> 2], 1u << pos);
          const uint32_t nh = (uint32_t)__popcll(__ballot(hit));
          j += nh;
          if (nh < 64u) break;
        }
        wave_lds_sync();
        lw = bm[lane];
        const uint32_t lc = (uint32_t)__popc(lw), li = wave_incl_scan(lc);
        // listed calls at the stored bases before word w: on a forward read those walked before it; on a reverse read all of them but the
        // ones at w and behind it (every entry is placed unless the list runs over, and then the call fields are never read)
        before = rev ? t_n - (j0 + li) : j0 + li - lc;
        if (rev) lw = __brev(lw);
        occ += cnt;
      }
      // (non-temporal: the entries are written once here and read by the decoder passes much later; through the cache they only
      // displace the SEQ and the rank lists the builder is still reading)
      if (k < nw) {
        const u32x2 vb = {lo[jj], hi[jj]}, vc = {lw, before};
        __builtin_nontemporal_store(vc, pl_call + w); __builtin_nontemporal_store(vb, pl_base + w);
      }
    }
  }
  // a delta list runs past the base's last occurrence (mod_bam.rs:705-727) iff the walk leaves entries unplaced: MKP_RF_RUNOVER, and the
  // record contributes coverage only (its call fields are never read)
  if (calls && j < t_n) flags |= MKP_RF_RUNOVER;
  if (__any(seqn)) flags |= MKP_RF_SEQN;
  if (lane == 0) {
    if (flags != h.flags) work[widx].flags = flags;
    if (flags & MKP_RF_SEQN) atomicAdd(seqn_bytes, (unsigned long long)min((L + 1u) >> 1, h.n_ent));
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// mkp_decode_slots: MM/ML decode + threshold caller + coverage, slot-driven (see the head of the file).
// Reference: DeltaListConverter (mod_bam.rs:667-733), get_base_mod_probs (1213-1295), combine_checked (629-656),
// into_collapsed (530-627), MultipleThresholdModCaller::call (threshold_mod_caller.rs:28-63), ReadCache::add_record
// (read_cache.rs:111-211), get_aligned_pairs_forward (util.rs:122-145), process_region's alignment loop (pileup/mod.rs:783-939).
// One wave runs one read start to end.  The per-slot instruction count matters (about 170 M VALU per C3 pass): the SEQ and the rank list
// were resolved into the two planes when the shard became resident (mkp_call_plane), so that a slot learns whether a call is listed there
// and as which call from one 8-byte gather and a popcount, and its base — needed only where no call is listed — from one dword more; the
// caller is resolved to a fixed walk per read.  No per-read LDS beyond the caller constants and no base windows: reads of every length take
// the same code.  The kernel sits between its issue rate and its memory traffic (profiles/strand_slots_c3.txt part 5), and two thirds of
// that traffic was the one 16-byte plane entry per slot, half of it base codes that a slot with a listed call never looks at: hence the
// split (profiles/split_plane_c3.txt).
// With every step waiting in full for its gather and then for its ML bytes a wave was parked on s_waitcnt for 70 % of its life (SQ counters,
// C3, eight waves per SIMD) and the kernel ran well short of its issue rate.  The slot loop is therefore a two-deep software pipeline
// over the 64-slot steps — A: map, request the plane gather; B: request the ML bytes; C: call, feature byte — run as B(s), A(s + 1),
// C(s), so that the ML bytes of step s travel under the mapping of step s + 1 and the gather of step s + 1 under the caller of step s (the
// comment at the loop has the details).  As it stands the kernel is bound by VALU issue again (profiles/decode_pipeline_c3.txt): what pays
// now is fewer instructions per step, not more overlap.
#define FUSED_PARAMS(PRM) const MkpWork* __restrict__ work, uint32_t n_reads, const uint32_t* __restrict__ cigar, const uint16_t* __restrict__ cigar16, \
    const uint8_t* __restrict__ seqs, \
    const MkpCallEnt* __restrict__ call_plane, const MkpBaseEnt* __restrict__ base_plane, const uint8_t* __restrict__ ml, const MkpFusedDesc* __restrict__ fdesc, PRM prm, const MkpSlotEnt* __restrict__ slot_ent, \
    uint8_t* __restrict__ cov, MkpVisit* __restrict__ visits, MkpReadOut* __restrict__ readout
#define FUSED_PASS work, n_reads, cigar, cigar16, seqs, call_plane, base_plane, ml, fdesc, prm, slot_ent, cov, visits, readout
__device__ __forceinline__ void decode_slots_body(FUSED_PARAMS(const MkpRunParams&), SlotLds* __restrict__ lds_all) {
  const int lane = lane_id();
  const uint32_t wib = rfl(threadIdx.x >> 6);
  const uint32_t widx = rfl(blockIdx.x * (blockDim.x >> 6)) + wib;
  if (widx >= n_reads) return;
  const MkpWork h = work[widx];
  SlotLds& W = lds_all[wib];
  const bool rev = (h.flags & MKP_RF_REVERSE) != 0;
  const uint32_t aln = rev ? 1u : 0u;
  const uint32_t L = h.l_seq;
  // the read's ops: 16 bits each, or its BAM words when one of them does not fit (the work record's offset is into the array it reads)
  const bool cg_wide = (h.flags & MKP_RF_CIGW) != 0;
  MkpCigarPtr cg = cg_wide ? (MkpCigarPtr)(cigar + h.cigar_off) : (MkpCigarPtr)(cigar16 + h.cigar_off);
  asm volatile("" : "+s"(cg));   // (one pointer: left to itself the compiler keeps both arrays' addresses through the slot loop)
  // a read with a base that is not A/C/G/T takes its bases from the SEQ (its offset; ~0 for every other read: one scalar register)
  const uint32_t seqn_off = (h.flags & MKP_RF_SEQN) ? h.seq_off : 0xffffffffu;
  bool have_calls = !(h.flags & MKP_RF_BAD) && h.n_tags != 0;
  // combine_checked's sum test (mod_bam.rs:629-656) — two tags on one base: the probabilities of a call add up to more than 1.01 — is
  // made by the host planner over the ML bytes (the f32 sums are exact multiples of 1/512: an integer comparison); a delta list that runs
  // past the last occurrence of its base (mod_bam.rs:705-727) by mkp_call_plane
  const bool err_rec = (h.flags & (MKP_RF_SUMERR | MKP_RF_RUNOVER)) != 0;
  // the slots this read answers: its run of a slot-entry list — its own strand's, or every slot's (MkpWork.ent_off) — {position, global slot
  // index} per entry; byte k of its stream run is global slot gs0 + k, so an entry's feature byte goes to cov[cov_off - gs0 + index]
  const uint32_t n_ent = h.n_ent, cov_rel = h.cov_off - h.gs0;
  const MkpSlotEnt* __restrict__ ents = slot_ent + h.ent_off;
  uint2 p_next = (uint32_t)lane < n_ent ? ldo<uint2>(ents, 8u * (uint32_t)lane) : make_uint2(0u, 0u);
  CigarWin rw; cigwin_init(rw, cg, cg_wide, h.n_cigar, h.ref_start);

  // ---- the read's one (mod strand, base) group.  The caller's walk over a call's map in iteration order is resolved once per
  // layout by the host (MkpFusedDesc: one scalar load): where the ML byte of the i-th code sits (tag + index: offset and stride
  // per call), its pass threshold and the counter of Modified(code).  --ignore / --preset traditional (ReDistribute) keep the
  // general tables.
  const bool collapse = prm.numeric_mode == 2;
  uint32_t fmisc = 0, f_col = 0;
  int32_t i_can = 0;   // Canonical's threshold in units of 2^-11 (the exact integer form of the caller, below); the codes' are in W.ck_thr
  // where the ML byte of the i-th code of call j sits: ml[W.ck_off[i] + j * W.ck_str[i]] (tag + index inside the tag: offset and stride)
  uint32_t mlx_o = 0, mlx_s = 0;
  uint32_t t_n = 0;
  if (have_calls) {
    t_n = h.n_calls;
    const MkpFusedDesc fd = fdesc[h.layout];
    fmisc = fd.misc; i_can = fd.i_can;
    if (lane < MKP_KMAX) {
      // the ML byte of a code the layout does not have is that of its last code: B requests two bytes, or four, C reads n_post of them
      const int lk = min(lane, (int)max((fd.misc >> 3) & 7u, 1u) - 1);
      const uint32_t src = (fd.it_src >> (4 * lk)) & 15u, tg = src & 1u;
      W.ck_off[lane] = (tg ? h.ml_off1 : h.ml_off0) + (src >> 1); W.ck_str[lane] = (fd.nc >> (8u * tg)) & 0xffu;
      W.ck_thr[lane] = lane == 0 ? fd.i_thr[0] : lane == 1 ? fd.i_thr[1] : lane == 2 ? fd.i_thr[2] : fd.i_thr[3];
      W.ck_cid[lane] = (fd.it_cid >> (8 * lane)) & 0xffu;
    }
    if (collapse) {
      f_col = fd.col;
      const uint32_t src = (fd.col >> 1) & 15u, tg = src & 1u;
      mlx_o = (tg ? h.ml_off1 : h.ml_off0) + (src >> 1); mlx_s = (fd.nc >> (8u * tg)) & 0xffu;
    }
    if (t_n == 0) have_calls = false;   // a tag without calls: the record has no modified-base information
  }
  const uint32_t sg0u = (fmisc >> 2) & 1u, n_post = (fmisc >> 3) & 7u;
  const bool int_caller = (fmisc >> (collapse ? 7 : 6)) & 1u;     // the exact integer form of the caller applies (fused_desc)
  const uint32_t red_shift = (f_col >> 5) & 3u;                   // log2 of the number of codes a collapsed code's probability is shared among
#ifdef MKP_DEBUG
  if (prm.debug_skip & 256u) have_calls = false;   // ablation: no calls (the read as if it had none)
#endif
  if (have_calls && err_rec) have_calls = false;   // the record only contributes coverage (skip_set, read_cache.rs:272-277)
#ifdef MKP_DEBUG
  const bool plane_calls = have_calls && !(prm.debug_skip & 128u);   // ablation: no calls (the base is still read from the plane)
#else
  const bool plane_calls = have_calls;
#endif
  // The plane the slot gather reads: a read with calls takes its call entries ({listed, before}) and asks the base plane for a dword only
  // under a match slot without a listed call; every other read (no tags, a tag without calls, BAD, SUMERR, RUNOVER) takes its base entries
  // ({base_lo, base_hi}) and never touches the call plane.  One pointer, uniform over the wave, chosen here and pinned as cg is: left to
  // itself the compiler carries both and selects at every gather.
  typedef const __attribute__((address_space(1))) char* MkpPlanePtr;
  MkpPlanePtr pl_base = (MkpPlanePtr)(base_plane + h.pad);
  MkpPlanePtr pl = plane_calls ? (MkpPlanePtr)(call_plane + h.pad) : pl_base;
  asm volatile("" : "+s"(pl), "+s"(pl_base));   // (pl_base too: unpinned, its loads take a 64-bit vector address, not `scalar base + offset`)

  // ---- the read's slots, 64 per step
  bool gaps = false; uint32_t n_callfeat = 0;
#ifdef MKP_DEBUG
  const uint32_t n_ent_walk = (prm.debug_skip & 512u) ? 0u : n_ent;   // ablation: no slot loop
#else
  const uint32_t n_ent_walk = n_ent;
#endif
  // The loop is a software pipeline, two steps deep.  A step is three stages:
  //   A(s)  reference -> query of the step's 64 slots (cigwin_map), then the plane gather pe(s) — 8 bytes per lane from the read's plane:
  //         the call plane for a read with calls, the base plane for every other — and the slot entries of step s + 1 (one 8-byte request
  //         per lane: position and global index) are requested.
  //         Both addresses are unconditional — clamped into the read's own plane / slot run — and the entry is masked where it is
  //         used: a load under a divergent branch is waited for on the spot.
  //   B(s)  `listed` and the call ordinal from pe(s), then the ML bytes of the step's calls, the base-plane dword of its match slots without
  //         a listed call (and the SEQ byte of a SEQN read) are requested; a step without a listed call requests no ML byte, one without
  //         an unlisted match slot no base.  What C needs of the slot is packed into one register (st).  (A read without calls has its
  //         bases in pe(s) and forms the coverage feature here.)
  //   C(s)  the caller on the ML bytes, NoCall(base) from the base dword, the feature byte, `gaps` / `n_callfeat`.  The byte is stored in B(s + 1), behind its requests (and
  //         behind the loop for the last step): the wait for pe(s + 1) at the head of the next iteration is a full one — the compiler
  //         counts the loop's entry edge, where nothing follows the gather — and a store issued just before it would be waited for.
  // A(0) runs in front of the loop; an iteration runs B(s), A(s + 1), C(s): the ML round trip of step s passes under the mapping of step
  // s + 1 — the longest VALU and LDS stretch of an iteration — and the gather of step s + 1 under the caller of step s.  Loads return in
  // issue order, so the wait in front of C(s) is a counted one that leaves pe(s + 1) and the slot positions in flight.  A(s + 1) runs
  // behind the last step as well (every lane invalid: no mapping, two loads of addresses inside the read's rooms): a branch around it would
  // make that wait a full drain.  Carried across A(s + 1): the ML bytes, the base dword, the SEQ byte and st; across C(s): pe(s + 1), kind, q.
  const uint32_t pl_last = max(MKP_PLANE_WORDS(L), 1u) - 1u, sq_last = (max(L, 1u) - 1u) >> 1, ent_last = max(n_ent, 1u) - 1u;
  uint32_t kind = 2u, q = 0u, fb_prev = 0u, g_cur = 0u, g_prev = 0u;
  typedef uint32_t U2 __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) U2* PlaneP2; typedef const __attribute__((address_space(1))) uint32_t* PlaneP1;
  U2 pe = {0u, 0u};
  auto stage_a = [&](uint32_t s0) {
    const uint32_t i = s0 + (uint32_t)lane;
    const bool valid = i < n_ent;
    const int32_t p = (int32_t)p_next.x;
    g_cur = p_next.y;
    // (the index leaves the loaded pair here: left where the scheduler puts it, the copy keeps the pair alive past the next request, the
    //  request in front of the loop lands in other registers, and the copy back is a wait on the loop's entry edge that nothing follows)
    asm volatile("" : "+v"(g_cur));
#ifdef MKP_DEBUG
    if (prm.debug_skip & 64u) { kind = 0u; q = min((uint32_t)(p - h.ref_start), L - 1u); } else   // ablation: no CIGAR mapping
#endif
    cigwin_map(rw, cg, cg_wide, h.n_cigar, h.ref_start, valid, p, &kind, &q);
    // the entry of the base in the read's plane (pl).  A read with calls: bit q & 31 of .listed = a listed call sits here, .before + the
    // listed bits below it = its stored-order ordinal; every other read: the 2-bit code of the base
    pe = *reinterpret_cast<PlaneP2>(pl + 8u * min(q >> 5, pl_last));
    p_next = ldo<uint2>(ents, 8u * min(i + 64u, ent_last));   // (behind the gather: see the wait for pe at the head of B)
  };
  // (ST_Q2: twice the base's index in its dword of the base plane, 2 * (q & 15): the shift that brings its code down)
  enum : uint32_t { ST_QODD = 1u << 8, ST_MATCH = 1u << 9, ST_LISTED = 1u << 10, ST_BASE = 1u << 11, ST_Q2_SHIFT = 12u };
  if (n_ent_walk != 0u) stage_a(0u);
  for (uint32_t s0 = 0; s0 < n_ent_walk; s0 += 64u) {
    const uint32_t i = s0 + (uint32_t)lane;
    const bool valid = i < n_ent;
    // ---- B(s)
    // (pe(s) and the slot entries were requested back to back: both are waited for here, in front of the ML requests, not behind them)
    asm volatile("" : "+v"(p_next.x), "+v"(p_next.y));
    uint32_t st;   // the coverage feature byte | ST_*
    uint32_t mlb[MKP_KMAX] = {0u, 0u, 0u, 0u}, mlx = 0, seq_byte = 0, base_dw = 0;
    {
      const bool is_match = valid && kind == 0u && q < L;
      if (plane_calls) {
        // pe = {listed, before}.  A deletion's feature and "not in the column" (a ref-skip, an entry past the read's last, a match past
        // the SEQ: a CIGAR longer than SEQ is refused by the packer) need no base; a match slot's feature is formed in C, from its call or,
        // without a listed one, from the dword of the base plane requested here.
        st = (valid && kind == 1u) ? feat(MKP_C_DEL, aln) : MKP_FB_NONE;
        const uint32_t qb = q & 31u;
        const bool listed = is_match && ((pe.x >> qb) & 1u);
        const bool want_base = is_match && !listed;
        if (__any(listed)) {
          // calls are listed in forward order: a reverse read's stored ordinal j is call n_calls - 1 - j
          const uint32_t jrel = pe.y + (uint32_t)__popc(pe.x & ((1u << qb) - 1u));
          const uint32_t jl = listed ? (rev ? t_n - 1u - jrel : jrel) : 0u;
          // All ML bytes of the call are requested before any is looked at (round 5 waited for each in turn: two to five dependent
          // memory round trips per 64 slots, the longest chain of the wave's life).
          const uint4 off4 = *reinterpret_cast<const uint4*>(W.ck_off), str4 = *reinterpret_cast<const uint4*>(W.ck_str);
          // Two requests, or four: a branch per code made the compiler join the paths with copies of the loaded registers, each behind a
          // wait of its own.  The entry of a code the read does not have repeats the read's last code (the caller constants above).
          auto mlq = [&](uint32_t o, uint32_t st_k) { return (uint32_t)ldo<uint8_t>(ml, __umul24(jl, st_k) + o); };
          mlb[0] = mlq(off4.x, str4.x); mlb[1] = mlq(off4.y, str4.y);
          if (n_post > 2u) { mlb[2] = mlq(off4.z, str4.z); mlb[3] = mlq(off4.w, str4.w); }
          if (f_col & 1u) mlx = (uint32_t)ldo<uint8_t>(ml, __umul24(jl, mlx_s) + mlx_o);
          if (listed) st |= ST_LISTED;
        }
        // The base of a match slot without a listed call: the dword of the read's base plane that holds base q, beside the ML requests and
        // of their shape — unconditional within a uniform test, every other lane's address the read's first dword (hot in cache), the
        // value masked where it is used.  Slots with a listed call never ask: on a read whose slots are mostly listed the base plane's
        // lines stay in HBM.
        if (__any(want_base)) {
          // (8 (q >> 5) + 4 ((q >> 4) & 1), clamped with a min: a select of the offset against 0 is widened to 64 bits, and the load then takes a
          //  64-bit vector address instead of `scalar base + 32-bit offset`)
          base_dw = *reinterpret_cast<PlaneP1>(pl_base + min((q >> 2) & ~3u, want_base ? 0xffffffffu : 0u));
          if (want_base) st |= ST_BASE | ((q & 15u) << (ST_Q2_SHIFT + 1u));
        }
      } else {
        // pe = {base_lo, base_hi}: the base is at hand
        const uint32_t code = (((q & 16u) ? pe.y : pe.x) >> (2u * (q & 15u))) & 3u;
        uint32_t fb = cover_feature(valid ? kind : 2u, 1u << code, aln);   // (the BAM code of the base is one-hot for A/C/G/T)
        if (valid && kind == 0u && q >= L) fb = MKP_FB_NONE;   // (a CIGAR longer than SEQ is refused by the packer)
        st = fb;
      }
      // a SEQN read's base comes from its SEQ byte, so that a non-ACGT base stays one
      if (seqn_off != 0xffffffffu) {
        seq_byte = (uint32_t)ldo<uint8_t>(seqs, seqn_off + min(q >> 1, sq_last));
        st |= ((q & 1u) ? ST_QODD : 0u) | (is_match ? ST_MATCH : 0u);
      }
    }
    // the feature bytes of step s - 1 leave here, behind the ML requests: by the next wait for a gather the store is a whole iteration old
    // (at its own slot's place in the read's run: g_prev is the global index of step s - 1, g_cur that of step s until A(s + 1) replaces it)
    if (i - 64u < n_ent) cov[cov_rel + g_prev] = (uint8_t)fb_prev;
    g_prev = g_cur;
    // ---- A(s + 1)
    stage_a(s0 + 64u);
    // ---- C(s)
    uint32_t call_fb = 0xffffffffu;
    {
      const bool listed = (st & ST_LISTED) != 0u;
      if (__any(listed)) {
        // MultipleThresholdModCaller::call (threshold_mod_caller.rs:28-63) on the map of this call, entries in the map's
        // iteration order: pass threshold, Iterator::max keeps the last maximum, canonical pushed last.  ReDistribute runs
        // (--ignore, --preset traditional) first add the collapsed code's share to every entry (mod_bam.rs:558-600).
        uint32_t cid = MKP_C_FAIL;
        if (int_caller) {
          // The same walk in integers, exactly: q -> (q + 0.5) / 256 is a multiple of 2^-9, the share of a collapsed code (its
          // probability over 1, 2 or 4 codes) a multiple of 2^-11, every sum of up to five of them and 1 - sum are exact in f32 — so
          // the f32 comparisons of the reference are comparisons of integers in units of 2^-11, thresholds rounded up to the next
          // multiple by the host (fused_desc: the least integer T with T / 2048 >= threshold).  One straight-line instance per number
          // of codes (uniform switch): no per-code masks held in scalar registers.
          const int4 thr4 = *reinterpret_cast<const int4*>(W.ck_thr);
          const uint4 cid4 = *reinterpret_cast<const uint4*>(W.ck_cid);
          const int32_t red4 = (f_col & 1u) ? (int32_t)(((2u * mlx + 1u) << 2) >> red_shift) + 4 : 4;
          int32_t sum = 0, best = INT32_MIN;
          auto step = [&](uint32_t b, int32_t thr, uint32_t c) {
            const int32_t v = (int32_t)(b << 3) + red4;
            sum += v;
            const bool take = v >= max(thr, best);   // passes, and no entry before it is larger (the last maximum wins)
            cid = take ? c : cid; best = take ? v : best;
          };
          switch (n_post) {
            case 1: step(mlb[0], thr4.x, cid4.x); break;
            case 2: step(mlb[0], thr4.x, cid4.x); step(mlb[1], thr4.y, cid4.y); break;
            case 3: step(mlb[0], thr4.x, cid4.x); step(mlb[1], thr4.y, cid4.y); step(mlb[2], thr4.z, cid4.z); break;
            case 4: step(mlb[0], thr4.x, cid4.x); step(mlb[1], thr4.y, cid4.y); step(mlb[2], thr4.z, cid4.z); step(mlb[3], thr4.w, cid4.w); break;
            default: break;
          }
          const int32_t pc = 2048 - sum;
          if (pc >= max(i_can, best)) cid = (fmisc >> 8) & 0xffu;
        // (a share over three codes: the f32 walk; its thresholds are read here — this is the rare path — not held in registers by every read)
        } else {
        const MkpFusedDesc& fdr = fdesc[h.layout];
        float f_thr[MKP_KMAX]; const float thr_can = fdr.thr_can;
#pragma unroll
        for (int k = 0; k < MKP_KMAX; k++) f_thr[k] = fdr.it_thr[k];
        float red = 0.f;
        if (f_col & 1u) red = (((float)mlx + 0.5f) / 256.0f) / fdr.n_other;
        float s = 0.f, best_p = 0.f; bool have = false;
#pragma unroll
        for (int k = 0; k < MKP_KMAX; k++) {
          if ((uint32_t)k < n_post) {
            float pr = ((float)mlb[k] + 0.5f) / 256.0f;   // quals_to_probs (mod_bam.rs:808-816)
            if (f_col & 1u) pr = pr + red;
            s = s + pr;
            const bool take = pr >= f_thr[k] && (!have || !(pr < best_p));
            cid = take ? W.ck_cid[k] : cid; best_p = take ? pr : best_p; have = have || take;
          }
        }
        const float pc = 1.0f - s;
        if (pc >= thr_can && (!have || !(pc < best_p))) cid = (fmisc >> 8) & 0xffu;
        }
        if (listed) call_fb = feat(cid, aln ^ sg0u);   // FeatureVector::add_feature's tally (pileup/mod.rs:238-281)
      }
    }
    uint32_t fb = st & 0xffu;
    // NoCall(base) of a match slot without a listed call, from the base plane's dword (the code complemented on a reverse read: cover_feature)
    if (st & ST_BASE) { const uint32_t code = (base_dw >> ((st >> ST_Q2_SHIFT) & 30u)) & 3u; fb = feat((uint32_t)MKP_C_NC + (aln ? 3u - code : code), aln); }
    if (seqn_off != 0xffffffffu && (st & ST_MATCH)) {
      const uint32_t nib = (st & ST_QODD) ? (seq_byte & 15u) : (seq_byte >> 4); fb = cover_feature(0u, nib, aln); }
    // (a scalar count: no per-lane counter, no scan at the end)
    { const bool cf = call_fb != 0xffffffffu; if (cf) fb = call_fb; n_callfeat += (uint32_t)__popcll(__ballot(cf)); }
    fb_prev = fb;
    gaps = gaps || (valid && fb == MKP_FB_NONE);
  }
  if (n_ent_walk != 0u) { const uint32_t i = ((n_ent_walk - 1u) & ~63u) + (uint32_t)lane; if (i < n_ent) cov[cov_rel + g_prev] = (uint8_t)fb_prev; }
  gaps = __any(gaps);
  const bool ok = have_calls;
  const uint32_t tally = aln ^ sg0u, ob_const = fmisc >> 16;
  const uint32_t n_cf = n_callfeat;
  if (lane == 0) {
    // (what the records below need of the work record is read again here rather than held in scalar registers through the slot loop)
    const MkpWork* hp = work + widx; asm volatile("" : "+s"(hp));
    const uint32_t h_gs0 = hp->gs0, h_n_sl = hp->n_sl, h_flags = hp->flags, h_cov_off = hp->cov_off, h_rid = hp->rid;
    MkpVisit v; v.gs0 = h_gs0; v.n_sl = h_n_sl; v.cov_off = h_cov_off;
    v.flags = (ok ? MKP_VF_OK : 0u) | (rev ? MKP_VF_REV : 0u) | (gaps ? MKP_VF_GAPS : 0u) | ((h_flags >> MKP_RF_KEY_SHIFT) << 8);
    v.obs0 = (ok && tally == 0u) ? ob_const : 0u; v.obs1 = (ok && tally == 1u) ? ob_const : 0u;
    v.over_off = 0; v.n_over = 0;
    visits[h_rid] = v;
    MkpReadOut out; out.n_events = ok ? n_cf : 0u; out.ok = ok ? 1u : 0u; out.obs[0] = v.obs0; out.obs[1] = v.obs1;
    readout[h_rid] = out;
  }
}

// Residency on gfx950 is also bounded by the SIMD's 800 scalar registers: a wave is charged ceil(sgprs / 16) * 16 + 16 of them
// (MI355X_MICROARCH.md, "Residency and cooperative launch"), so a kernel left to take 105 admits six waves per SIMD whatever the LDS and
// VGPR budgets say.  The decoder is capped at 80 — eight waves.
#ifndef MKP_DECODE_SGPRS
#define MKP_DECODE_SGPRS 80
#endif
extern "C" __global__ void __attribute__((amdgpu_num_sgpr(MKP_DECODE_SGPRS))) __launch_bounds__(256) mkp_decode_slots(FUSED_PARAMS(MkpRunParams)) {
  __shared__ __attribute__((aligned(16))) SlotLds lds_all[4]; decode_slots_body(FUSED_PASS, lds_all); }

// ----------------------------------------------------------------------------------------------------------------------
// mkp_cover_reads: coverage features of the reads the event-producing decode kernels handled, with their call events merged in.
// An event's counter id / tally strand are those the decode kernels computed; the first event on a position (bit 12) replaces the
// NoCall of the base, a second one (pos_call and neg_call on one base, pileup/mod.rs:889-938) goes to the read's overflow list —
// written over the front of its own event slice, which holds only events already consumed.
extern "C" __global__ void __launch_bounds__(256) mkp_cover_reads(const MkpReadHdr* __restrict__ hdrs, uint32_t n_reads,
    const uint32_t* __restrict__ read_ids, const uint32_t* __restrict__ cigar, const uint8_t* __restrict__ seqs,
    const uint32_t* __restrict__ slot_pos, uint8_t* __restrict__ cov, MkpVisit* __restrict__ visits, MkpEvent* __restrict__ events,
    MkpReadOut* __restrict__ readout) {
  __shared__ uint32_t stage_all[4][64];
  const int lane = lane_id();
  const uint32_t wib = rfl(threadIdx.x >> 6);
  const uint32_t widx = rfl(blockIdx.x * (blockDim.x >> 6)) + wib;
  if (widx >= n_reads) return;
  const uint32_t rid = rfl(read_ids[widx]);
  const MkpReadHdr h = hdrs[rid];
  const MkpReadOut ro = readout[rid];
  uint32_t* __restrict__ stage = stage_all[wib];
  const bool rev = (h.flags & MKP_RF_REVERSE) != 0;
  const uint32_t aln = rev ? 1u : 0u, L = h.l_seq;
  const uint8_t* __restrict__ seqb = seqs + h.seq_off;
  const MkpCigarPtr cg = (MkpCigarPtr)(cigar + h.cigar_off);   // (the BAM words: `wide`)
  const bool ok = ro.ok == 1u;
  const uint32_t n_ev = ok ? ro.n_events : 0u;
  MkpEvent* __restrict__ ev = events + h.event_off;
  const uint32_t n_sl = h.n_sl, gs0 = h.gs0;
  uint8_t* __restrict__ covp = cov + h.cov_off;
  CigarWin rw; cigwin_init(rw, cg, true, h.n_cigar, h.ref_start);
  uint32_t p_next = (uint32_t)lane < n_sl ? slot_pos[gs0 + (uint32_t)lane] : 0u;
  uint32_t ec = 0, n_over = 0; bool gaps = false;
  stage[lane] = 0xffffffffu;
  for (uint32_t s0 = 0; s0 < n_sl; s0 += 64) {
    const uint32_t i = s0 + (uint32_t)lane; const bool valid = i < n_sl;
    const int32_t p = (int32_t)p_next;
    { const uint32_t in = i + 64u; p_next = in < n_sl ? slot_pos[gs0 + in] : 0u; }
    uint32_t kind, q;
    cigwin_map(rw, cg, true, h.n_cigar, h.ref_start, valid, p, &kind, &q);
    const bool is_match = valid && kind == 0u && q < L;
    const uint32_t byte = is_match ? (uint32_t)seqb[q >> 1] : 0u;
    const uint32_t nib = (q & 1u) ? (byte & 15u) : (byte >> 4);
    uint32_t fb = cover_feature(valid ? kind : 2u, nib, aln);
    if (valid && kind == 0u && q >= L) fb = MKP_FB_NONE;
    if (ec < n_ev) {
      // the read's events up to the step's last slot position, 64 at a time; each finds the lane holding its position
      const uint32_t nval = min(64u, n_sl - s0);
      const uint32_t pkey = valid ? (uint32_t)p : 0xffffffffu;
      const uint32_t p_hi = (uint32_t)__builtin_amdgcn_readlane((int)pkey, (int)(nval - 1u));
      wave_lds_sync();
      for (;;) {
        const uint32_t k = ec + (uint32_t)lane; const bool in = k < n_ev;
        MkpEvent e; e.pos = 0xffffffffu; e.info = 0;
        if (in) e = ev[k];
        const bool take = in && e.pos <= p_hi;
        const int tgt = find_sorted(pkey, take ? e.pos : 0u);
        const uint32_t tp = (uint32_t)__shfl((int)pkey, tgt & 63, 64);
        const bool match = take && tgt < 64 && tp == e.pos;
        const uint32_t eb = feat(e.info & 0x1fu, (e.info >> 8) & 1u);
        const bool prim = match && (e.info & (1u << 12)), over = match && !(e.info & (1u << 12));
        if (prim) stage[tgt] = eb;
        const unsigned long long ob = __ballot(over);
        if (over) { MkpEvent o; o.pos = gs0 + s0 + (uint32_t)tgt; o.info = eb; ev[n_over + (uint32_t)__popcll(ob & lanemask_lt())] = o; }
        n_over += (uint32_t)__popcll(ob);
        const uint32_t nt = (uint32_t)__popcll(__ballot(take));
        ec += nt;
        if (nt < 64u) break;
      }
      wave_lds_sync();
      const uint32_t sv = stage[lane];
      if (sv != 0xffffffffu) { fb = sv; stage[lane] = 0xffffffffu; }
    }
    if (valid) covp[i] = (uint8_t)fb;
    gaps = gaps || (valid && fb == MKP_FB_NONE);
  }
  gaps = __any(gaps);
  if (lane == 0) {
    MkpVisit v; v.gs0 = gs0; v.n_sl = n_sl; v.cov_off = h.cov_off;
    v.flags = (ok ? MKP_VF_OK : 0u) | (rev ? MKP_VF_REV : 0u) | (gaps ? MKP_VF_GAPS : 0u) | ((h.flags >> MKP_RF_KEY_SHIFT) << 8);
    v.obs0 = ok ? ro.obs[0] : 0u; v.obs1 = ok ? ro.obs[1] : 0u;
    v.over_off = h.event_off; v.n_over = n_over;
    visits[rid] = v;
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// mkp_pileup_stream: accumulate + emit over the feature stream.  LDS: the regions of StreamLds (mkp_dev_rows.hpp) — packed strand tallies
// per counter and observed-code slot (WIDE — the _wide kernels, for shards whose deepest column may hold more than 65 535 records — one
// u32 plane per strand instead), the tile's slot positions, a word per slot for the emission and the row map.  Waves draw the tile's
// candidate reads from an LDS ticket; a visit = the read's MkpVisit (scalar loads), its bytes for the tile's slots (a dword per lane), one
// LDS atomic per feature.  Observed codes: +1 / -1 at the ends of the read's slot range (and at every change between covered and not
// covered when the read holds ref-skips).  Rows: emit_stream_rows (mkp_dev_rows.hpp); MkpRunParams is resolved once per workgroup into a
// small table (StreamProg) so that the emission does not walk slot lists.
// The body reads top to bottom: prologue, then per round of candidates compaction and visits, the observed-code scans, the rows.

// What does not hang on the tile's ticket: the tallies are cleared (their size is a kernel argument), the parameter block and the combos
// come in.  Callers put a barrier behind it.
__device__ __forceinline__ void stream_prologue(uint32_t* __restrict__ lds, uint32_t tal_words, const MkpRunParams* __restrict__ prmp,
    uint32_t* __restrict__ prm_lds, const MkpCombo* __restrict__ combos, uint32_t n_combos, uint32_t* __restrict__ combo_lds) {
  const uint32_t nv = tal_words >> 2; uint4* l4 = reinterpret_cast<uint4*>(lds);
  for (uint32_t k = threadIdx.x; k < nv; k += PILEUP_THREADS) l4[k] = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t k = (nv << 2) + threadIdx.x; k < tal_words; k += PILEUP_THREADS) lds[k] = 0;
  for (uint32_t kq = threadIdx.x; kq < sizeof(MkpRunParams) / 4; kq += PILEUP_THREADS) prm_lds[kq] = reinterpret_cast<const uint32_t*>(prmp)[kq];
  for (uint32_t kq = threadIdx.x; kq < n_combos * (sizeof(MkpCombo) / 4); kq += PILEUP_THREADS) combo_lds[kq] = reinterpret_cast<const uint32_t*>(combos)[kq];
}

// Where a feature of (counter `row`, tally strand `st`) is tallied: the byte offset of its LDS row (S4 = 4 * S) and the increment.  Narrow:
// one multiply for the row, one multiply-add for the increment (1 or 1 << 16); WIDE: 1 on the strand's plane 2 * counter + strand.
struct TallyAt { uint32_t off, inc; };
template <bool WIDE> __device__ __forceinline__ TallyAt tally_at(uint32_t row, uint32_t st, uint32_t S4) {
  if (WIDE) return {(uint32_t)__umul24(2u * row + st, S4), 1u};
  return {(uint32_t)__umul24(row, S4), __umul24(st, 0xffffu) + 1u};
}

// one visit: the read's bytes for this tile's slots (first dword per lane already in `wcur`), its observed codes, its overflow events
template <bool KEYED, bool WIDE>
__device__ __forceinline__ void stream_visit(const MkpVisit& v, uint32_t wcur, const StreamLds& L, const MkpSTile& tl, uint32_t n_oslots,
    uint32_t key_filter, const uint8_t* __restrict__ cov, const MkpEvent* __restrict__ events) {
  const int lane = lane_id();
  const uint32_t gh0 = tl.gh0, gh1 = tl.gh1, n_tslots = gh1 - gh0, S = L.S, S4 = S * 4u, talbase = lds_addr(L.tal);
  uint32_t* __restrict__ obs = L.obs;
  const uint32_t a = max(v.gs0, gh0), b = min(v.gs0 + v.n_sl, gh1);
  if (a >= b) return;
  if (KEYED && (v.flags >> 8) != key_filter) return;   // --partition-tag: one pass per key
  const uint32_t k_lo = a - v.gs0, k_hi = b - v.gs0;      // the read's bytes for this tile
  const uint32_t col0 = v.gs0 - gh0;                      // column of byte k = col0 + k (mod 2^32)
  const uint8_t* __restrict__ cp = cov + v.cov_off;
  const uint32_t kfirst = (k_lo & ~3u) + 4u * (uint32_t)lane;
  // observed mod codes over the columns the read is in (add_mod_codes_for_record, pileup/mod.rs:831-835)
  if ((v.flags & MKP_VF_OK) && (v.obs0 | v.obs1)) {
    // one lane per (observed-code slot, tally strand): +1 where the read enters the tile's columns, -1 behind its last
    if (!(v.flags & MKP_VF_GAPS)) {
      const uint32_t sl = (uint32_t)lane >> 1, st = (uint32_t)lane & 1u;
      if (sl < n_oslots && (((st ? v.obs1 : v.obs0) >> sl) & 1u)) obs_diff<WIDE>(obs, S, sl, st, a - gh0, b - gh0, n_tslots, false);
    } else {   // ref-skips: the read is not in those columns (alignment.is_refskip()) — a change of state per boundary
      for (uint32_t k = k_lo + (uint32_t)lane; k <= k_hi; k += 64) {
        const bool cur = k < k_hi && cp[k] != MKP_FB_NONE, prev = k > k_lo && cp[k - 1u] != MKP_FB_NONE;
        const uint32_t col = col0 + k;
        if (cur != prev && col < n_tslots) for (uint32_t s = 0; s < 2; s++) {
          uint32_t m = s ? v.obs1 : v.obs0;
          const uint32_t inc = WIDE ? 1u : s ? 0x10000u : 1u;
          while (m) { const uint32_t sl = (uint32_t)__ffs((int)m) - 1u; m &= m - 1u;
            atomicAdd(&obs[(WIDE ? 2u * sl + s : sl) * S + col], cur ? inc : 0u - inc); }
        }
      }
    }
  }
  // bytes outside [k_lo, k_hi) — the ends of the read's first and last dword in this tile — become "no feature": the first dword's (lane 0 of
  // the first round only) once per visit, the last dword's once per round
  uint32_t lom = kfirst < k_lo ? ~(0xffffffffu << (8u * (k_lo - kfirst))) : 0u;
  for (uint32_t k = kfirst;; k += 256u) {
    uint32_t w = wcur | lom;
    lom = 0;
    const uint32_t kn = k + 256u;
    wcur = kn < k_hi ? *reinterpret_cast<const uint32_t*>(cp + kn) : 0xffffffffu;
    if (k + 4u > k_hi) w |= k >= k_hi ? 0xffffffffu : 0xffffffffu << (8u * (k_hi - k));
    const uint32_t lane_base = talbase + 4u * (col0 + k);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      // feature byte: [0:4] counter, [5] tally strand, >= 0x40 none.  One multiply-add for the row address (the byte's column goes into the
      // instruction's offset field), one for the increment (tally_at)
      if (!(w & (0xc0u << (8u * j)))) {
        const TallyAt t = tally_at<WIDE>((w >> (8u * j)) & 31u, (w >> (8u * j + 5u)) & 1u, S4);
        lds_u32* col = (lds_u32*)(uintptr_t)(lane_base + t.off);
        __hip_atomic_fetch_add(col + j, t.inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    if (!__any(kn < k_hi)) break;
  }
  for (uint32_t k = (uint32_t)lane; k < v.n_over; k += 64) {   // second features on one column
    const MkpEvent e = events[v.over_off + k];
    const TallyAt t = tally_at<WIDE>(e.info & 31u, (e.info >> 5) & 1u, S4);
    if (e.pos >= gh0 && e.pos < gh1) lds_add(talbase + 4u * (e.pos - gh0) + t.off, t.inc);
  }
}

// The tile's candidate reads [first, last) are a superset (everything that starts before the tile's end and behind the longest read's reach:
// about half of them end before the tile starts, C3).  Every thread looks at one candidate of the round that starts at c0 — slot range
// only, one 8-byte load — and the ones that reach into the tile are compacted into a list in LDS (the row map's words: the emission is not
// running yet).  Returns the length of the list; the barriers around it are inside.
template <bool KEYED>
__device__ __forceinline__ uint32_t stream_candidates(const MkpVisit* __restrict__ visits, uint32_t c0, const MkpSTile& tl, uint32_t key_filter,
    uint32_t* __restrict__ list, uint32_t* next_read, uint32_t* n_real) {
  // (the round before is through with the list)
  if (c0 != tl.first) { __syncthreads(); if (threadIdx.x == 0) { *next_read = 0; *n_real = 0; } __syncthreads(); }
  const uint32_t cnd = c0 + threadIdx.x; bool reaches = false;
  if (cnd < tl.last) {
    const uint2 gr = *reinterpret_cast<const uint2*>(&visits[cnd]);   // gs0, n_sl
    reaches = max(gr.x, tl.gh0) < min(gr.x + gr.y, tl.gh1);
    if (KEYED && reaches) reaches = (visits[cnd].flags >> 8) == key_filter;   // --partition-tag: one pass per key
  }
  const unsigned long long bal = __ballot(reaches);
  uint32_t w0 = 0; if (lane_id() == 0 && bal) w0 = atomicAdd(n_real, (uint32_t)__popcll(bal));
  w0 = rfl(w0);
  if (reaches) list[w0 + (uint32_t)__popcll(bal & lanemask_lt())] = cnd;
  __syncthreads();
  return *n_real;
}
// The waves draw from that list, VB at a time: the visit records and the first stream dword of each are requested before any of them is
// used (a visit is a chain ticket -> 32-byte record -> one dword per lane -> LDS atomics).  With the emission row-major the visits are
// the kernel — 0.077 of 0.133 ms (profiles/r06_stream_ablation.txt) — and every empty candidate used to cost a ticket, a scalar load and its wait.
template <bool KEYED, uint32_t VB, bool WIDE>
__device__ __forceinline__ void stream_draw_visits(const MkpVisit* __restrict__ visits, uint32_t n_here, const StreamLds& L, const MkpSTile& tl,
    uint32_t n_oslots, uint32_t key_filter, const uint8_t* __restrict__ cov, const MkpEvent* __restrict__ events, uint32_t* next_read) {
  const int lane = lane_id();
  for (;;) {
    uint32_t base; { uint32_t ticket = 0; if (lane == 0) ticket = atomicAdd(next_read, VB); base = rfl(ticket); }
    if (base >= n_here) break;
    MkpVisit vv[VB]; uint32_t ww[VB];
#pragma unroll
    for (uint32_t j = 0; j < VB; j++) vv[j] = visits[rfl(L.rowmap[min(base + j, n_here - 1u)])];   // (uniform: scalar loads)
#pragma unroll
    for (uint32_t j = 0; j < VB; j++) {
      const uint32_t a = max(vv[j].gs0, tl.gh0), b = min(vv[j].gs0 + vv[j].n_sl, tl.gh1);
      const uint32_t k_lo = a - vv[j].gs0, k_hi = b - vv[j].gs0, kfirst = (k_lo & ~3u) + 4u * (uint32_t)lane;
      ww[j] = (a < b && kfirst < k_hi) ? *reinterpret_cast<const uint32_t*>(cov + vv[j].cov_off + kfirst) : 0xffffffffu;
    }
#pragma unroll
    for (uint32_t j = 0; j < VB; j++) if (base + j < n_here) stream_visit<KEYED, WIDE>(vv[j], ww[j], L, tl, n_oslots, key_filter, cov, events);
  }
}

template <bool KEYED, uint32_t VB /* visits drawn per ticket, their records and first stream dwords requested together */, bool WIDE = false>
__device__ __forceinline__ void pileup_stream_body(const MkpVisit* __restrict__ visits, const uint8_t* __restrict__ cov,
    const MkpEvent* __restrict__ events,
                 const MkpSTile* __restrict__ tiles, uint32_t n_tiles, const MkpRunParams* __restrict__ prmp, const uint32_t* __restrict__ slot_pos,
                 const uint8_t* __restrict__ focus, const MkpCombo* __restrict__ combos, uint32_t* __restrict__ rows_base,
                     uint32_t* __restrict__ row_cursor,
                 uint32_t* __restrict__ tile_row_off, uint32_t* __restrict__ dev_err, uint32_t key_arg, uint32_t n_combos, uint32_t n_runs,
                     uint32_t S, uint32_t tal_words) {
  const uint32_t key_filter = KEYED ? (key_arg & 0xffffu) : 0u, key_run = key_arg >> 16;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t next_read, n_real, run_ticket, row_base_s, row_total_s;
  __shared__ uint32_t wave_tot[PILEUP_WAVES];
  __shared__ __attribute__((aligned(16))) uint32_t prm_lds[(sizeof(MkpRunParams) + 3) / 4];
  __shared__ __attribute__((aligned(16))) uint32_t combo_lds[64 * sizeof(MkpCombo) / 4];
  __shared__ StreamProg prog;
  // ---- prologue
  // A workgroup takes the next TILE from an atomic ticket (row_cursor[0]; the host zeroes it before the first pass), not from blockIdx: rows
  // leave in genome order through a look-back over the runs before (mkp_dev_rows.hpp), and a run may only wait for runs whose workgroups
  // are already running — true for tickets whatever the dispatch order, with any number of contexts on the device.
  // The prologue is a chain of memory round trips in front of the first tally — ticket, tile record, visit records, stream dwords.  What does
  // not hang on it starts beside the ticket (stream_prologue); the slot positions and focus bytes (needed by the emission only) are
  // requested when the tile is known and land in LDS behind the visits.  ONE barrier stands between a workgroup's start and its first visit.
  if (threadIdx.x == 0) { run_ticket = atomicAdd(row_cursor, 1u); next_read = 0; n_real = 0; }
  stream_prologue(lds, tal_words, prmp, prm_lds, combos, n_combos, combo_lds);
  __syncthreads();
  const MkpRunParams& prm = *reinterpret_cast<const MkpRunParams*>(prm_lds);
  const uint32_t n_counters = rfl(prm.n_counters), n_oslots = rfl(prm.n_slots);
  const StreamLds L = {lds, lds + n_counters * S * (WIDE ? 2u : 1u), reinterpret_cast<int32_t*>(lds + tal_words), lds + tal_words + S,
      lds + tal_words + 2u * S, S};
  const uint32_t run = rfl(run_ticket);   // row-run index: key pass * tiles + tile (passes run one after the other on the stream)
  const uint32_t tix = run - key_run * n_tiles;
  if (tix >= n_tiles) { if (threadIdx.x == 0) atomicOr(dev_err, ERR_ROW_CAP); return; }   // (cannot happen: one ticket per workgroup)
  const MkpSTile tl = tiles[tix];   // (uniform: scalar loads)
  const uint32_t n_tslots = tl.gh1 - tl.gh0;
  // this thread's slot: position now, focus byte behind the visits
  int32_t my_pos = 0;
  if (threadIdx.x < n_tslots) my_pos = (int32_t)slot_pos[tl.gh0 + threadIdx.x];
  rowprog_build(prm, n_counters, prog);   // (threads 0..15; read after the visits' barrier)
  // ---- candidates and visits, PILEUP_THREADS candidates per round
  for (uint32_t c0 = tl.first; c0 < tl.last; c0 += PILEUP_THREADS) {
#ifdef MKP_DEBUG
    if (prm.debug_skip & 1024u) break;   // ablation: no visits (prologue + scans + emission only)
#endif
    const uint32_t n_here = stream_candidates<KEYED>(visits, c0, tl, key_filter, L.rowmap, &next_read, &n_real);
    stream_draw_visits<KEYED, VB, WIDE>(visits, n_here, L, tl, n_oslots, key_filter, cov, events, &next_read);
  }
  // the emission's per-slot words: position and focus byte (the byte's load overlaps the barrier and the scans below)
  uint32_t my_fv = 0;
  if (threadIdx.x < n_tslots) { L.fpos[threadIdx.x] = my_pos; my_fv = prm.has_focus ? (uint32_t)focus[my_pos - prm.win_start] : 3u; }
  __syncthreads();
  // ---- scans: observed-code difference arrays -> counts, in place and still packed (WIDE: one array per strand plane)
  for (uint32_t a = rfl(threadIdx.x >> 6); a < (WIDE ? 2u * n_oslots : n_oslots); a += PILEUP_WAVES) prefix_sum_in_place(L.obs + a * S, n_tslots);
  if (threadIdx.x < n_tslots) L.aux[threadIdx.x] = my_fv;
  __syncthreads();
  // ---- rows
  emit_stream_rows<WIDE>(L, n_counters, tl, my_pos, my_fv, run, n_runs, key_filter, prm, prog, reinterpret_cast<const MkpCombo*>(combo_lds),
      rows_base, row_cursor, tile_row_off, dev_err, wave_tot, &row_base_s, &row_total_s);
}

#define STREAM_PARAMS const MkpVisit* __restrict__ visits, const uint8_t* __restrict__ cov, const MkpEvent* __restrict__ events, const MkpSTile* __restrict__ tiles, uint32_t n_tiles, \
    const MkpRunParams* __restrict__ prmp, const uint32_t* __restrict__ slot_pos, const uint8_t* __restrict__ focus, const MkpCombo* __restrict__ combos, uint32_t* __restrict__ rows_base, \
    uint32_t* __restrict__ row_cursor, uint32_t* __restrict__ tile_row_off, uint32_t* __restrict__ dev_err, uint32_t key_arg, uint32_t n_combos, uint32_t n_runs, uint32_t S, uint32_t tal_words
#define STREAM_PASS visits, cov, events, tiles, n_tiles, prmp, slot_pos, focus, combos, rows_base, row_cursor, tile_row_off, dev_err, key_arg, n_combos, n_runs, S, tal_words
#ifndef MKP_STREAM_VB
#define MKP_STREAM_VB 4
#endif
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_stream(STREAM_PARAMS) {
  pileup_stream_body<false, MKP_STREAM_VB>(STREAM_PASS); }
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_stream_keyed(STREAM_PARAMS) {
  pileup_stream_body<true, MKP_STREAM_VB>(STREAM_PASS); }
// shards whose deepest column may hold more than 65 535 records: u32 tallies per strand (tal_words = twice the narrow kernels')
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_stream_wide(STREAM_PARAMS) {
  pileup_stream_body<false, MKP_STREAM_VB, true>(STREAM_PASS); }
extern "C" __global__ void __launch_bounds__(PILEUP_THREADS, 8) mkp_pileup_stream_keyed_wide(STREAM_PARAMS) {
  pileup_stream_body<true, MKP_STREAM_VB, true>(STREAM_PASS); }

// ----------------------------------------------------------------------------------------------------------------------
// Records sharing a read name inside one interval (MkpDupCons / MkpDupSeg, mkp_device.h).  Rare: a handful of records per shard.
//   mkp_dup_restore  before the decode kernels: a consumer's header points at its OWN event slice again (a re-launch on a resident shard finds
//                    it pointing at the rebuilt list of the pass before)
//   mkp_dup_events   after the decode kernels: one wave per consumer rebuilds its event list segment by segment.  Own segment: its events are
//                    copied.  Foreign segment: the owner's events in the segment's positions — each is a (reference position, counter, mod
//                    strand, base) of the OWNER's call map — are kept where the consumer's own alignment has a base at that position and the
//                    base (read orientation) is the call's base (get_mod_call asks `calls[strand][read_base].get(position)`, read_cache.rs:232-297),
//                    with the tally strand of the consumer's alignment (add_feature, pileup/mod.rs:238-281).
//   mkp_dup_apply    the consumer's header / summary now describe the rebuilt list: cover / accumulate kernels take it as the record's own.
// The observed codes and the status (skip set, read_cache.rs:272-277) are the owner's too; the accumulate kernels apply ONE set per record, so
// owners that disagree across a consumer's segments raise ERR_DUP_MIXED (the host refuses the shard) instead of being approximated.
extern "C" __global__ void __launch_bounds__(64) mkp_dup_restore(MkpReadHdr* __restrict__ hdrs, const MkpDupCons* __restrict__ cons, uint32_t n) {
  const uint32_t k = blockIdx.x * 64u + threadIdx.x;
  if (k < n) hdrs[cons[k].rid].event_off = cons[k].own_off;
}
extern "C" __global__ void __launch_bounds__(64) mkp_dup_apply(MkpReadHdr* __restrict__ hdrs, MkpReadOut* __restrict__ readout,
    const MkpDupCons* __restrict__ cons, uint32_t n) {
  const uint32_t k = blockIdx.x * 64u + threadIdx.x;
  if (k >= n) return;
  const MkpDupCons c = cons[k];
  hdrs[c.rid].event_off = c.eff_off;
  MkpReadOut o; o.n_events = c.out_n; o.ok = c.out_ok; o.obs[0] = c.out_obs0; o.obs[1] = c.out_obs1;
  readout[c.rid] = o;
}
extern "C" __global__ void __launch_bounds__(64) mkp_dup_events(const MkpReadHdr* __restrict__ hdrs, const uint32_t* __restrict__ cigar,
    const uint8_t* __restrict__ seqs, MkpEvent* __restrict__ events,
                                                                const MkpReadOut* __restrict__ readout, MkpDupCons* __restrict__ cons,
                                                                    const MkpDupSeg* __restrict__ segs, uint32_t n, uint32_t* __restrict__ dev_err) {
  const uint32_t ci = blockIdx.x;
  if (ci >= n) return;
  const int lane = lane_id();
  const MkpDupCons c = cons[ci];
  const MkpReadHdr h = hdrs[c.rid];
  const uint32_t aln = (h.flags & MKP_RF_REVERSE) ? 1u : 0u, L = h.l_seq;
  const uint8_t* __restrict__ seqb = seqs + h.seq_off;
  const MkpCigarPtr cg = (MkpCigarPtr)(cigar + h.cigar_off);   // (the BAM words: `wide`)
  CigarWin rw; cigwin_init(rw, cg, true, h.n_cigar, h.ref_start);
  MkpEvent* __restrict__ dst = events + c.eff_off;
  uint32_t n_out = 0, st_ok = 0, st_o0 = 0, st_o1 = 0; bool have_st = false, mixed = false, over = false;
  for (uint32_t s = 0; s < c.n_seg; s++) {
    const MkpDupSeg sg = segs[c.seg_off + s];
    const MkpReadOut ro = readout[sg.owner];   // (the owner's own summary: mkp_dup_apply runs behind this kernel)
    const uint32_t ok = ro.ok == 1u ? 1u : 0u, o0 = ok ? ro.obs[0] : 0u, o1 = ok ? ro.obs[1] : 0u;
    if (!have_st) { st_ok = ok; st_o0 = o0; st_o1 = o1; have_st = true; } else if (ok != st_ok || o0 != st_o0 || o1 != st_o1) mixed = true;
    const uint32_t n_src = ok ? ro.n_events : 0u;
    const MkpEvent* __restrict__ src = events + sg.src_off;
    const bool own = sg.owner == c.rid;
    for (uint32_t at = event_lower_bound(src, n_src, sg.p_lo);; at += 64u) {
      const uint32_t k = at + (uint32_t)lane;
      MkpEvent e; e.pos = 0xffffffffu; e.info = 0;
      if (k < n_src) e = src[k];
      const bool in = k < n_src && (int32_t)e.pos < sg.p_hi;
      bool keep = in;
      if (!own) {
        // the consumer's own alignment at the call's reference position: a base (M / = / X), and the call's base in read orientation
        uint32_t kind = 2u, q = 0u;
        const bool inside = in && (int32_t)e.pos >= h.ref_start && (int32_t)e.pos < h.ref_end;
        cigwin_map(rw, cg, true, h.n_cigar, h.ref_start, inside, (int32_t)e.pos, &kind, &q);
        keep = false;
        if (inside && kind == 0u && q < L) {
          const uint32_t byte = (uint32_t)seqb[q >> 1], nib = (q & 1u) ? (byte & 15u) : (byte >> 4);
          const int sb = nib2base(nib);
          const uint32_t rb = sb < 0 ? 4u : (aln ? 3u - (uint32_t)sb : (uint32_t)sb);
          keep = rb == ((e.info >> 9) & 3u);
        }
        // the mod strand of the owner's call (its tally strand seen from its own alignment), tallied from THIS record's alignment strand
        const uint32_t mod_strand = ((e.info >> 8) ^ (e.info >> 11)) & 1u;
        e.info = (e.info & ~((1u << 8) | (1u << 11))) | ((aln ^ mod_strand) << 8) | (aln << 11);
      }
      const unsigned long long bk = __ballot(keep);
      const uint32_t nk = (uint32_t)__popcll(bk);
      if (n_out + nk > c.eff_cap) { over = true; break; }
      if (keep) dst[n_out + (uint32_t)__popcll(bk & lanemask_lt())] = e;
      n_out += nk;
      if (!__all(in)) break;
    }
    if (over) break;
  }
  if (lane == 0) {
    if (mixed) atomicOr(dev_err, ERR_DUP_MIXED);
    if (over) atomicOr(dev_err, ERR_EVENT_CAP);
    MkpDupCons* o = cons + ci;
    o->out_n = st_ok ? n_out : 0u; o->out_ok = st_ok; o->out_obs0 = st_o0; o->out_obs1 = st_o1;
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// host-side launchers (declared in mkp_launch.h)
// work = the fused decoder's reads (longest first), cover_ids = the reads of mkp_cover_reads
// (call_plane, base_plane: the fused reads' two planes, MkpWork.pad indexes both)
extern "C" hipError_t mkp_launch_slots(hipStream_t st, const MkpWork* work, uint32_t n_fused, const MkpCallEnt* call_plane, const MkpBaseEnt* base_plane,
    const MkpShardArrays& sh, const uint32_t* cover_ids, uint32_t n_cover, const MkpFusedDesc* fdesc, const MkpRunParams* prm,
    const uint32_t* slot_pos, const MkpSlotEnt* slot_ent, uint8_t* cov, MkpVisit* visits) {
  if (n_fused) hipLaunchKernelGGL(mkp_decode_slots, dim3((n_fused + 3u) / 4u), dim3(256), 0, st, work, n_fused, sh.cigar, sh.cigar16, sh.seq, call_plane,
      base_plane, sh.ml, fdesc, *prm, slot_ent, cov, visits, sh.readout);
  if (n_cover) hipLaunchKernelGGL(mkp_cover_reads, dim3((n_cover + 3u) / 4u), dim3(256), 0, st, sh.hdr, n_cover, cover_ids, sh.cigar, sh.seq, slot_pos, cov,
      visits, sh.events, sh.readout);
  return hipGetLastError();
}
// the call plane and the base plane of the fused reads (once per resident shard; it also marks the work records whose delta list runs past its base
// and those with a base that is not A/C/G/T, and adds the SEQ bytes the decoder reads of the latter to *seqn_bytes)
extern "C" hipError_t mkp_launch_call_plane(hipStream_t st, MkpWork* work, uint32_t n_fused, const MkpShardArrays& sh, const MkpFusedDesc* fdesc,
    MkpCallEnt* call_plane, MkpBaseEnt* base_plane, unsigned long long* seqn_bytes) {
  if (n_fused) hipLaunchKernelGGL(mkp_call_plane, dim3((n_fused + 3u) / 4u), dim3(256), 0, st, work, n_fused, sh.seq, sh.ranks, fdesc, call_plane,
      base_plane, seqn_bytes);
  return hipGetLastError();
}

extern "C" hipError_t mkp_launch_dup_restore(hipStream_t st, const MkpShardArrays& sh, const MkpDupCons* cons, uint32_t n) {
  if (n) hipLaunchKernelGGL(mkp_dup_restore, dim3((n + 63u) / 64u), dim3(64), 0, st, sh.hdr, cons, n);
  return hipGetLastError();
}
extern "C" hipError_t mkp_launch_dup_events(hipStream_t st, const MkpShardArrays& sh, MkpDupCons* cons, const MkpDupSeg* segs, uint32_t n,
    uint32_t* dev_err) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(mkp_dup_events, dim3(n), dim3(64), 0, st, sh.hdr, sh.cigar, sh.seq, sh.events, sh.readout, cons, segs, n, dev_err);
  hipLaunchKernelGGL(mkp_dup_apply, dim3((n + 63u) / 64u), dim3(64), 0, st, sh.hdr, sh.readout, cons, n);
  return hipGetLastError();
}

extern "C" hipError_t mkp_stream_set_lds(uint32_t bytes) {
  for (const void* k : {(const void*)mkp_pileup_stream, (const void*)mkp_pileup_stream_keyed, (const void*)mkp_pileup_stream_wide,
                        (const void*)mkp_pileup_stream_keyed_wide}) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" hipError_t mkp_launch_stream(hipStream_t st, uint32_t lds_bytes, const MkpVisit* visits, const uint8_t* cov, const MkpEvent* events,
    const MkpSTile* tiles, uint32_t n_tiles,
                                        const MkpRunParams* prm_dev, const uint32_t* slot_pos, const uint8_t* focus, const MkpCombo* combos,
                                            const MkpRowsDev* rows, uint32_t* row_cursor,
                                        uint32_t* tile_row_off, uint32_t* dev_err, uint32_t key_filter, uint32_t key_slot,
                                            uint32_t n_combos, uint32_t n_runs, uint32_t slot_cap, uint32_t words_per_slot, bool wide) {
  if (!n_tiles) return hipSuccess;
  const bool keyed = key_filter != MKP_NO_KEY_FILTER;
  const uint32_t key_arg = keyed ? ((key_filter & 0xffffu) | (key_slot << 16)) : 0u;
#define MKP_STREAM_LAUNCH(K) hipLaunchKernelGGL(K, dim3(n_tiles), dim3(PILEUP_THREADS), lds_bytes, st, visits, cov, events, tiles, n_tiles, prm_dev, slot_pos, focus, combos, rows->pos, row_cursor, \
                                                tile_row_off, dev_err, key_arg, n_combos > 64u ? 64u : n_combos, n_runs, slot_cap, words_per_slot * slot_cap)
  // ONE build per kernel: a one-shot shard pass and a re-launch on the resident shard run the same code object
  // wide shards: words_per_slot counts both strand planes
  if (wide) { if (keyed) MKP_STREAM_LAUNCH(mkp_pileup_stream_keyed_wide); else MKP_STREAM_LAUNCH(mkp_pileup_stream_wide); }
  else if (keyed) MKP_STREAM_LAUNCH(mkp_pileup_stream_keyed); else MKP_STREAM_LAUNCH(mkp_pileup_stream);
  return hipGetLastError();
}
