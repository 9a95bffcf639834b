// Row emission from a tile's LDS tallies, for the accumulate kernels of mkp_kernels.hip and mkp_slots.hip:
//   the row program (StreamProg, stream_row_*, rowprog_build): FeatureVector::decode / add_tally_to_counts / combine_strand_features
//     (pileup/mod.rs:283-561) as a table per workgroup — both files;
//   what the three emitters share: rows_view (the row buffer's columns), block_excl_scan (a thread's place among the tile's rows),
//     store_row, rows_this_round;
//   emit_dense_rows: the tail of the dense mkp_pileup_tiles kernels;
//   StreamLds, lookback_reserve_wave, emit_stream_rows: the tail of the mkp_pileup_stream kernels, row runs in genome order (mkp_slots.hip);
//   hemi_rows_at, SlotMap, emit_hemi_rows: the tail of mkp_pileup_tiles_hemi (DuplexFeatureVector::decode, duplex.rs:124-205);
//   obs_diff, prefix_sum_in_place (observed codes as difference arrays), lds_add, event_lower_bound: small device helpers both files use.
#pragma once
#include "mkp_dev_common.hpp"

#define PILEUP_THREADS MKP_PILEUP_THREADS
#define PILEUP_WAVES (PILEUP_THREADS / 64)
#define PILEUP_WAVE_SCRATCH MKP_PILEUP_WAVE_SCRATCH

struct RowAcc { uint32_t n_valid, n_mod, n_can, n_other, n_del, n_fail, n_diff, n_nocall; };

// the row buffer as columns: 11 SoA arrays of row_capacity entries behind rows_base
__device__ __forceinline__ MkpRowsDev rows_view(uint32_t* __restrict__ q, size_t cap) {
  MkpRowsDev rows;
  rows.pos = q; rows.info = q + cap; rows.code = q + 2 * cap; rows.n_valid = q + 3 * cap; rows.n_mod = q + 4 * cap; rows.n_can = q + 5 * cap;
  rows.n_other = q + 6 * cap; rows.n_del = q + 7 * cap; rows.n_fail = q + 8 * cap; rows.n_diff = q + 9 * cap; rows.n_nocall = q + 10 * cap;
  return rows;
}
__device__ __forceinline__ void store_row(const MkpRowsDev& rows, size_t at, uint32_t pos, uint32_t info, uint32_t code, const RowAcc& acc) {
  rows.pos[at] = pos; rows.info[at] = info; rows.code[at] = code;
  rows.n_valid[at] = acc.n_valid; rows.n_mod[at] = acc.n_mod; rows.n_can[at] = acc.n_can; rows.n_other[at] = acc.n_other;
  rows.n_del[at] = acc.n_del; rows.n_fail[at] = acc.n_fail; rows.n_diff[at] = acc.n_diff; rows.n_nocall[at] = acc.n_nocall;
}
// Block exclusive scan of a per-thread row count (thread order = row order): returns the rows of the threads before this one, *total = the
// tile's rows.  wave_tot: a word of LDS per wave.  One barrier inside, between the waves' totals and their sum; a caller that runs it
// again, or reuses wave_tot, puts its own barrier in between.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t cnt, uint32_t* wave_tot, uint32_t* total) {
  const uint32_t wave = threadIdx.x >> 6, incl = wave_incl_scan(cnt);
  if (lane_id() == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t off = incl - cnt, tot = 0;
  for (uint32_t w2 = 0; w2 < PILEUP_WAVES; w2++) { const uint32_t t = wave_tot[w2]; if (w2 < wave) off += t; tot += t; }
  *total = tot;
  return off;
}
// rows are placed through a row map of `words` entries per round: the rows of the round that starts at row r0 of the tile
__device__ __forceinline__ uint32_t rows_this_round(uint32_t total, uint32_t r0, uint32_t words) {
  const uint32_t end = min(total, r0 + words);
  return end > r0 ? end - r0 : 0u;
}

// Observed code `sl` of tally strand `s` over the columns [a, b): +1 at a, -1 at b — an interval-OR as a difference array
// (`leave`: the reverse, a ref-skip inside the read's span).  Narrow: the strand's half of the packed word; WIDE: its plane.
template <bool WIDE>
__device__ __forceinline__ void obs_diff(uint32_t* __restrict__ obs, uint32_t S, uint32_t sl, uint32_t s, uint32_t a, uint32_t b, uint32_t n_tslots,
    bool leave) {
  uint32_t* __restrict__ row = obs + (WIDE ? 2u * sl + s : sl) * S;
  const uint32_t one = WIDE ? 1u : (s ? 0x10000u : 1u), v = leave ? 0u - one : one;
  atomicAdd(&row[a], v);
  if (b < n_tslots) atomicAdd(&row[b], 0u - v);
}
// difference array -> counts, in place, by one wave (packed halves stay exact: neither half ever goes negative in the sum)
__device__ __forceinline__ void prefix_sum_in_place(uint32_t* __restrict__ arr, uint32_t n) {
  const uint32_t lane = (uint32_t)lane_id();
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += 64) {
    const uint32_t v = (b0 + lane < n) ? arr[b0 + lane] : 0u;
    const uint32_t sc = wave_incl_scan(v);
    if (b0 + lane < n) arr[b0 + lane] = sc + carry;
    carry += (uint32_t)__builtin_amdgcn_readlane((int)sc, 63);
  }
}

// pileup-hemi rows of one '+' motif position whose counters sit in column i (DuplexFeatureVector::decode, duplex.rs:124-205, in the
// writer's order: primary base, then pattern — writers.rs:196-207).  The pattern goes out as its two element indices
// (rows.code = a | b << 8), the primary base in rows.info; the host turns the elements into mod codes.
template <bool WRITE>
__device__ __forceinline__ uint32_t hemi_rows_at(const uint32_t* __restrict__ tal, uint32_t S, const MkpRunParams& prm, int32_t p, uint32_t i,
    const MkpRowsDev& rows, uint32_t wr) {
  uint32_t tot[4], n = 0;
  for (int pb = 0; pb < 4; pb++) {
    tot[pb] = 0;
    const uint32_t base = prm.hemi_pat_base[pb], nel = prm.hemi_nel[pb];
    if (base != 0xffu) for (uint32_t k = 0; k < nel * nel; k++) tot[pb] += tal[(base + k) * S + i];
  }
  for (int pb = 0; pb < 4; pb++) {
    if (!tot[pb]) continue;
    const uint32_t base = prm.hemi_pat_base[pb], nel = prm.hemi_nel[pb];
    for (uint32_t k = 0; k < nel * nel; k++) {
      const uint32_t cnt = tal[(base + k) * S + i];
      if (!cnt) continue;
      if (WRITE) {
        const RowAcc acc = {tot[pb], cnt, tal[base * S + i], tot[pb] - cnt, tal[MKP_H_DEL * S + i], tal[(MKP_H_FAIL + pb) * S + i],
            tot[0] + tot[1] + tot[2] + tot[3] - tot[pb], tal[(MKP_H_NC + pb) * S + i]};
        store_row(rows, wr + n, (uint32_t)p, (uint32_t)pb, (k / nel) | ((k % nel) << 8), acc);
      }
      n++;
    }
  }
  return n;
}

// ----------------------------------------------------------------------------------------------------------------------
// Row emission, row-major: MkpRunParams resolved once per workgroup into a small table (the "row program"), existence of a row decided
// from a handful of tallies, one thread per ROW filling and storing it (mkp_pileup_stream, the dense mkp_pileup_tiles kernels).
// A "group" is one row candidate per strand (or per motif when strands combine): the observed-code slots in row order, or the four
// primary bases (--combine-mods).
struct StreamProg {
  uint32_t n_groups;
  uint32_t totmask;        // counters that add up to a column's total (all but Delete and Filtered)
  uint32_t modmask[4];     // primary base -> the counters of its mod codes
  uint32_t code[16];       // group -> code of its rows
  // group -> [0:1] primary base, [2:6] observed-code slot + 1 (0: a --combine-mods row), [7:11] counter of the code,
  // [12:16] counter of Canonical(base), [17] the base has one, [18] first group of its code (strand combining adds up the groups of a code)
  uint32_t info[16];
};

// Tally k of strand s in column i.  Narrow shards (every column at most 65 535 records deep): one u32 per (k, column), '+' in the low and
// '-' in the high 16 bits.  WIDE shards: one u32 plane per (k, strand), plane 2k + s.
template <bool WIDE = false>
__device__ __forceinline__ uint32_t col_get(const uint32_t* __restrict__ tal, uint32_t S, uint32_t i, uint32_t s, uint32_t k) {
  if (WIDE) return tal[(2u * k + s) * S + i];
  return (tal[k * S + i] >> (16u * s)) & 0xffffu; }
template <bool WIDE = false>
__device__ __forceinline__ uint32_t col_sum(const uint32_t* __restrict__ tal, uint32_t S, uint32_t i, uint32_t s, uint32_t mask) {
  uint32_t t = 0;
  while (mask) { const uint32_t k = (uint32_t)__ffs((int)mask) - 1u; mask &= mask - 1u; t += col_get<WIDE>(tal, S, i, s, k); }
  return t;
}
// does (strand tally s, column i, group g) yield a row — add_tally_to_counts's early returns (pileup/mod.rs:283-410): the primary base has
// filtered coverage, and (per-code rows) the code was observed in a record over this column
template <bool WIDE = false>
__device__ __forceinline__ bool stream_row_exists(const uint32_t* __restrict__ tal, uint32_t S, uint32_t n_counters, const StreamProg& P, uint32_t s,
    uint32_t i, uint32_t g) {
  const uint32_t inf = P.info[g];
  if (!((inf >> 17) & 1u)) return false;
  const uint32_t cov = col_get<WIDE>(tal, S, i, s, (inf >> 12) & 31u) + col_sum<WIDE>(tal, S, i, s, P.modmask[inf & 3u]);
  if (!cov) return false;
  const uint32_t osl = (inf >> 2) & 31u;
  return !osl || col_get<WIDE>(tal, S, i, s, n_counters + osl - 1u) != 0u;
}
// the row itself, added into `r`
template <bool WIDE = false>
__device__ __forceinline__ void stream_row_add(const uint32_t* __restrict__ tal, uint32_t S, const StreamProg& P, uint32_t s, uint32_t i, uint32_t g,
    RowAcc& r) {
  const uint32_t inf = P.info[g], pb = inf & 3u;
  const uint32_t n_can = col_get<WIDE>(tal, S, i, s, (inf >> 12) & 31u), mods = col_sum<WIDE>(tal, S, i, s, P.modmask[pb]);
  const uint32_t n_mod = ((inf >> 2) & 31u) ? col_get<WIDE>(tal, S, i, s, (inf >> 7) & 31u) : mods;
  const uint32_t total = col_sum<WIDE>(tal, S, i, s, P.totmask), nocall = col_get<WIDE>(tal, S, i, s, MKP_C_NC + pb), cov = n_can + mods;
  r.n_valid += cov; r.n_mod += n_mod; r.n_can += n_can; r.n_other += mods - n_mod;
  r.n_del += col_get<WIDE>(tal, S, i, s, MKP_C_DEL); r.n_fail += col_get<WIDE>(tal, S, i, s, MKP_C_FAIL);
  r.n_diff += total - (nocall + cov); r.n_nocall += nocall;
}

// the row program, built by threads 0..15 of the workgroup (callers put a barrier before its first use)
__device__ __forceinline__ void rowprog_build(const MkpRunParams& prm, uint32_t n_counters, StreamProg& prog) {
  if (threadIdx.x >= 16u) return;
  const uint32_t g = threadIdx.x, combine_mods = prm.numeric_mode == 1 ? 1u : 0u;
  const uint32_t ng = combine_mods ? 4u : prm.n_slots;
  uint32_t code = 0, inf = 0;
  if (g < ng) {
    const uint32_t sl = combine_mods ? 0u : prm.slot_order[g], pb = combine_mods ? g : prm.slots[sl].pb, ck = prm.can_of_pb[pb];
    code = combine_mods ? (uint32_t)"ACGT"[g] : prm.slots[sl].code_repr;
    const bool first = combine_mods || g == 0u || prm.slots[prm.slot_order[g - 1u]].code_repr != code;
    inf = pb | ((combine_mods ? 0u : sl + 1u) << 2) | ((combine_mods ? 0u
        : (uint32_t)prm.slots[sl].cid) << 7) | (((MKP_C_CAN + ck) & 31u) << 12) | ((ck != 0xffu ? 1u : 0u) << 17) | ((first ? 1u : 0u) << 18);
  }
  prog.code[g] = code; prog.info[g] = inf;
  if (g < 4u) { uint32_t m = 0; for (uint32_t t = 0; t < prm.n_slots; t++) if (prm.slots[t].pb == g) m |= 1u << prm.slots[t].cid; prog.modmask[g] = m;
    }
  if (g == 0u) { prog.n_groups = ng; prog.totmask = ((1u << n_counters) - 1u) & ~((1u << MKP_C_DEL) | (1u << MKP_C_FAIL)); }
}

// Rows of a DENSE tile (mkp_pileup_tiles without focus positions: every position of the tile's range owns a column, both strands of every
// position are candidates, strands never combine): each thread takes a contiguous run of columns — rows keep position order — counts its
// rows, the block scans, thread 0 reserves the tile's run of the row buffer (mkp_scan_tiles + mkp_gather_rows order the runs afterwards),
// the threads scatter (column, strand, group) words into `rowmap` (LDS, `map_words` dwords: the accumulate phase's per-wave scratch, dead
// by now) and then every thread fills and stores whole rows.  Existence is evaluated twice (count, scatter) — a handful of LDS reads —
// instead of keeping a mask per column.
template <bool WIDE>
__device__ __forceinline__ void emit_dense_rows(const uint32_t* __restrict__ tal, uint32_t S, uint32_t n_counters, uint32_t n_tslots, int32_t T0h,
    const MkpTile& tl, uint32_t run, uint32_t key,
                                                const MkpRunParams& prm, StreamProg& prog, uint32_t* __restrict__ rowmap, uint32_t map_words,
                                                    uint32_t* __restrict__ rows_base,
                                                uint32_t* __restrict__ row_cursor, uint32_t* __restrict__ tile_row_off,
                                                    uint32_t* __restrict__ tile_row_cnt, uint32_t* __restrict__ dev_err,
                                                uint32_t* wave_tot, uint32_t* row_base_p, uint32_t* row_total_p) {
  rowprog_build(prm, n_counters, prog);
  __syncthreads();
  const StreamProg& P = prog;
  // (strands combine at motif positions only: a run without focus positions has none)
  const uint32_t n_groups = prm.combine_strands ? 0u : P.n_groups;
  const uint32_t per = (n_tslots + PILEUP_THREADS - 1u) / PILEUP_THREADS;
  const uint32_t i0 = min(n_tslots, threadIdx.x * per), i1 = min(n_tslots, i0 + per);
  auto in_rows = [&](uint32_t i) { const int32_t p = T0h + (int32_t)i; return p >= tl.r0 && p < tl.r1; };
  uint32_t cnt = 0;
  for (uint32_t i = i0; i < i1; i++) {
    if (!in_rows(i)) continue;
    for (uint32_t s = 0; s < 2; s++) for (uint32_t g = 0; g < n_groups; g++) cnt += stream_row_exists<WIDE>(tal, S, n_counters, P, s, i, g) ? 1u : 0u;
  }
  uint32_t tile_rows;
  const uint32_t off = block_excl_scan(cnt, wave_tot, &tile_rows);
  if (threadIdx.x == 0) {
    uint32_t s = tile_rows;
    const uint32_t base = s ? atomicAdd(row_cursor, s) : 0u;
    if (base + s > prm.row_capacity) { atomicOr(dev_err, ERR_ROW_CAP); s = 0; }
    *row_base_p = base; *row_total_p = s; tile_row_off[run] = base; tile_row_cnt[run] = s;
  }
  const MkpRowsDev rows = rows_view(rows_base, prm.row_capacity);
  for (uint32_t r0 = 0; r0 < tile_rows; r0 += map_words) {
    if (r0) __syncthreads();   // the round before has read the map
    if (cnt && off < r0 + map_words && off + cnt > r0) {
      uint32_t r = off;
      for (uint32_t i = i0; i < i1; i++) {
        if (!in_rows(i)) continue;
        for (uint32_t s = 0; s < 2; s++) for (uint32_t g = 0; g < n_groups; g++) {
          if (!stream_row_exists<WIDE>(tal, S, n_counters, P, s, i, g)) continue;
          if (r >= r0 && r < r0 + map_words) rowmap[r - r0] = i | (g << 13) | (s << 17);
          r++;
        }
      }
    }
    __syncthreads();
    const uint32_t n_here = rows_this_round(*row_total_p, r0, map_words);
    for (uint32_t rr = threadIdx.x; rr < n_here; rr += PILEUP_THREADS) {
      const uint32_t e = rowmap[rr], si = e & 8191u, g = (e >> 13) & 15u, s = (e >> 17) & 1u;
      RowAcc acc = {0, 0, 0, 0, 0, 0, 0, 0};
      stream_row_add<WIDE>(tal, S, P, s, si, g, acc);
      // (no motif: info[8:15] = 0)
      store_row(rows, (size_t)*row_base_p + r0 + rr, (uint32_t)(T0h + (int32_t)si), s | (key << 16), P.code[g], acc);
    }
  }
}

// LDS byte addresses as integers: a tally update is then `lane base + 256*window + row*4*S`, two VALU instructions
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p; }
__device__ __forceinline__ void lds_add(uint32_t a, uint32_t v) {
  __hip_atomic_fetch_add((lds_u32*)(uintptr_t)a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// first index in the position-sorted event list `ev[0..n)` whose pos is >= key: 64-way probes, two dependent
// loads for up to 4096 events instead of a 12-step bisection
__device__ __forceinline__ uint32_t event_lower_bound(const MkpEvent* __restrict__ ev, uint32_t n, int32_t key) {
  const uint32_t lane = (uint32_t)lane_id();
  uint32_t lo = 0, span = n;
  while (span > 64) {
    const uint32_t stride = (span + 63u) >> 6;
    const uint32_t k = lo + lane * stride;
    const bool valid = k < lo + span;
    const int32_t p = valid ? (int32_t)ev[k].pos : 0x7fffffff;
    const uint32_t c = (uint32_t)__popcll(__ballot(valid && p < key));
    if (c == 0) return lo;
    const uint32_t nlo = lo + (c - 1u) * stride + 1u;
    const uint32_t nhi = min(lo + c * stride, lo + span);
    lo = nlo; span = nhi - nlo;
  }
  const bool valid = lane < span;
  const int32_t p = valid ? (int32_t)ev[lo + lane].pos : 0x7fffffff;
  return lo + (uint32_t)__popcll(__ballot(valid && p < key));
}

// Position <-> tally column of a pileup-hemi tile, where only the '+' motif positions own a column: a bitmap of the tile's (halo'd)
// range plus its running popcount (both in LDS) give rank(p) = number of such positions below p, which is the column of p when p
// is one, and the first column at or after p when it is not (what the ends of a read span or of a CIGAR window need).
struct SlotMap {
  const uint32_t* bm; const uint32_t* pfx; const int32_t* fpos; int32_t lbase;   // lbase: position of bit 0 of bm[0]
  __device__ __forceinline__ uint32_t rank(int32_t p) const {
    const uint32_t lb = (uint32_t)(p - lbase), w = lb >> 5;
    return pfx[w] + (uint32_t)__popc(bm[w] & ((1u << (lb & 31u)) - 1u));
  }
  __device__ __forceinline__ bool is_slot(int32_t p) const { const uint32_t lb = (uint32_t)(p - lbase); return (bm[lb >> 5] >> (lb & 31u)) & 1u; }
  __device__ __forceinline__ int32_t pos_of(uint32_t c) const { return fpos[c]; }
};

// Row runs of the slot pipeline (mkp_slots.hip) leave in genome order without a second pass: a run's place in the row buffer is the number of rows of the runs before it, found by
// a decoupled look-back over one 64-bit word per run (bits 62-63: 1 = this run's own count is known, 2 = the count of everything up to
// and including it; low bits: the value).  Run numbers are TICKETS drawn from an atomic counter when a workgroup starts (round 5; round 4
// took blockIdx and relied on dispatch order), so the runs a workgroup waits for belong to workgroups that are already running, whatever
// the dispatch order and whoever else shares the device.  The look-back is made by a whole wave, 64 words per step (round 4: one thread,
// one dependent global load per run before it — with 512 workgroups in flight that walk was most of a tile's tail).
__device__ __forceinline__ uint32_t lookback_reserve_wave(unsigned long long* __restrict__ state, uint32_t run, uint32_t s) {
  const int lane = lane_id();
  if (lane == 0) __hip_atomic_store(&state[run], (1ull << 62) | (unsigned long long)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t excl = 0;
  for (long long hi = (long long)run - 1; hi >= 0;) {
    const long long idx = hi - lane;
    // (before the first run: everything so far = 0)
    const unsigned long long v = idx >= 0 ? __hip_atomic_load(&state[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (2ull << 62);
    const uint32_t flag = (uint32_t)(v >> 62);
    const unsigned long long m2 = __ballot(flag == 2u), m0 = __ballot(flag == 0u);
    const uint32_t first2 = m2 ? (uint32_t)__builtin_ctzll(m2) : 64u, first0 = m0 ? (uint32_t)__builtin_ctzll(m0) : 64u;
    // the words nearest to this run, up to the first inclusive one or to the first that is not written yet
    const uint32_t take = first0 < first2 ? first0 : (first2 < 64u ? first2 + 1u : 64u);
    const uint32_t part = wave_incl_scan((uint32_t)lane < take ? (uint32_t)v : 0u);
    excl += (uint32_t)__builtin_amdgcn_readlane((int)part, 63);
    if (first2 < first0) break;          // reached a run that knows everything before it
    hi -= take;
    if (first0 < 64u) __builtin_amdgcn_s_sleep(2);   // the next word is still being counted
  }
  if (lane == 0) __hip_atomic_store(&state[run], (2ull << 62) | (unsigned long long)(excl + s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return excl;
}

// The dynamic LDS of a mkp_pileup_stream tile of S columns, region by region (carved by pileup_stream_body, mkp_slots.hip)
struct StreamLds {
  uint32_t* tal;      // [counter | observed-code slot][S] packed tallies ('+' in the low, '-' in the high 16 bits); WIDE: [..][strand][S]
  uint32_t* obs;      // the observed-code rows of `tal`: difference arrays while the reads are visited, counts behind the scans
  int32_t* fpos;      // [S] the tile's slot positions
  uint32_t* aux;      // [S] per slot: [0:7] focus byte, [8 + 6m ..] partner column of the m-th '+' motif (strand combining)
  uint32_t* rowmap;   // [MKP_STREAM_ROWMAP_WORDS] the candidate reads of a round while reads are visited, then the row map
  uint32_t S;
};

// Rows of a STREAM tile (the tail of the mkp_pileup_stream kernels; thread i holds slot i's position and focus word, the observed codes
// are counts by now):
//   E1  one thread per SLOT decides which rows exist: a bit per (strand | motif, code group) candidate — existence needs the coverage of
//       the candidate's primary base and its observed-code count, a handful of LDS reads — and counts them;
//   E2  block scan of the counts; wave 0 reserves the tile's run in the row buffer (decoupled look-back over the runs before, in ticket
//       order) while every thread scatters (slot, candidate) words of its rows into the ROW MAP in LDS;
//   E3  one thread per ROW fills its row from the tallies and stores it: every store instruction writes 64 consecutive rows of one column.
// (One thread per slot running a parameter-driven interpreter twice — count, then write — cost ~800 VALU instructions per thread, 29
// spilled registers, and wrote the rows of a slot with stride-2 stores.)
template <bool WIDE>
__device__ __forceinline__ void emit_stream_rows(const StreamLds& L, uint32_t n_counters, const MkpSTile& tl, int32_t my_pos, uint32_t my_fv,
    uint32_t run, uint32_t n_runs, uint32_t key, const MkpRunParams& prm, const StreamProg& P, const MkpCombo* combos_l,
    uint32_t* __restrict__ rows_base, uint32_t* __restrict__ row_cursor, uint32_t* __restrict__ tile_row_off, uint32_t* __restrict__ dev_err,
    uint32_t* wave_tot, uint32_t* row_base_p, uint32_t* row_total_p) {
  const uint32_t* __restrict__ tal = L.tal; const int32_t* __restrict__ fpos = L.fpos;
  uint32_t* __restrict__ aux = L.aux; uint32_t* __restrict__ rowmap = L.rowmap;
  const int lane = lane_id();
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t S = L.S, n_tslots = tl.gh1 - tl.gh0;
  // ---- E1: which rows does this thread's slot yield (FeatureVector::decode, pileup/mod.rs:412-446; combine_strand_features 469-561)
  const uint32_t n_groups = P.n_groups;
  const bool combine = prm.combine_strands != 0;
  const uint32_t i = threadIdx.x;
  unsigned long long em = 0; uint32_t cnt = 0, mult0 = 1, mult1 = 1;
#ifdef MKP_DEBUG
  const bool dbg_norows = (prm.debug_skip & 2048u) != 0;   // ablation: no rows (the look-back word is still published so that nothing waits)
#else
  constexpr bool dbg_norows = false;
#endif
  if (!dbg_norows && i < n_tslots && my_pos >= tl.r0 && my_pos < tl.r1 && (my_fv & 3u)) {
    const uint32_t rule = my_fv & 3u, combo = my_fv >> 2;
    if (!combine) {
      if (combo) { const MkpCombo& cb = combos_l[combo]; mult0 = cb.n_pos ? cb.n_pos : 1u; mult1 = cb.n_neg ? cb.n_neg : 1u; }
      for (uint32_t s = 0; s < 2; s++) {
        if (!((rule >> s) & 1u)) continue;
        for (uint32_t g = 0; g < n_groups; g++) if (stream_row_exists<WIDE>(tal, S, n_counters, P, s, i, g)) em |= 1ull << (16u * s + g);
      }
      cnt = (uint32_t)__popc((uint32_t)em & 0xffffu) * mult0 + (uint32_t)__popc((uint32_t)(em >> 16) & 0xffffu) * mult1;
    } else if (combo) {   // only '+' motif positions produce rows
      const MkpCombo& cb = combos_l[combo];
      const bool pos_ok = (rule & 1u) != 0;
      uint32_t part = 0;
      for (uint32_t m = 0; m < cb.n_pos; m++) {
        const int delta = cb.pos_delta[m];
        if (delta == -128) continue;   // not a palindrome / negative_strand_position() == None
        const int idx = cb.pos_ids[m];
        const int32_t qpos = my_pos + delta;
        bool neg_ok = false; uint32_t iq = i;
        if (delta != -127 && qpos >= prm.win_start && qpos < prm.win_end) {   // -127: the mate position is in another interval
          // the partner's column: a focus position at most MKP_HALO away — a few columns up or down
          if (delta > 0) { while (iq + 1u < n_tslots && fpos[iq + 1u] <= qpos) iq++; } else { while (iq > 0u && fpos[iq - 1u] >= qpos) iq--; }
          if (fpos[iq] == qpos) {
            const uint32_t fq = aux[iq] & 0xffu;
            if ((fq & 2u) && (fq >> 2)) { const MkpCombo& cq = combos_l[fq >> 2];
              for (uint32_t k = 0; k < cq.n_neg; k++) neg_ok |= (cq.neg_ids[k] == idx);
              }
          }
        }
        if (neg_ok) part |= ((iq - i + 32u) & 63u) << (8u + 6u * m);
        for (uint32_t g = 0; g < n_groups; g++) {
          if (!((P.info[g] >> 18) & 1u)) continue;   // grouped by code (BTreeMap)
          bool any = false;
          for (uint32_t gj = g; gj < n_groups && (gj == g || !((P.info[gj] >> 18) & 1u)); gj++)
            any = any || (pos_ok && stream_row_exists<WIDE>(tal, S, n_counters, P, 0, i, gj))
                || (neg_ok && stream_row_exists<WIDE>(tal, S, n_counters, P, 1, iq, gj));
          if (any) { em |= 1ull << (16u * m + g); cnt++; }
        }
      }
      if (part) aux[i] = my_fv | part;   // (own word; the other threads only look at the focus byte, which stays)
    }
  }
  // ---- E2: place of every slot's rows inside the tile, the tile's place in the row buffer
  uint32_t tile_rows;
  const uint32_t off = block_excl_scan(cnt, wave_tot, &tile_rows);
  const MkpRowsDev rows = rows_view(rows_base, prm.row_capacity);
  for (uint32_t r0 = 0; r0 == 0u || r0 < tile_rows; r0 += MKP_STREAM_ROWMAP_WORDS) {
    if (r0) __syncthreads();   // the round before has read the map
    // (slot, candidate) of every row of this round: [0:9] slot, [10:13] group, [14:15] strand | motif, [16:17] which of the position's motif ids
    if (cnt && off < r0 + MKP_STREAM_ROWMAP_WORDS && off + cnt > r0) {
      uint32_t r = off;
      for (uint32_t sm = 0; sm < 4u; sm++) {
        uint32_t bits = (uint32_t)(em >> (16u * sm)) & 0xffffu;
        const uint32_t mult = combine ? 1u : (sm ? mult1 : mult0);
        while (bits) {
          const uint32_t g = (uint32_t)__ffs((int)bits) - 1u; bits &= bits - 1u;
          for (uint32_t k = 0; k < mult; k++, r++) if (r >= r0
              && r < r0 + MKP_STREAM_ROWMAP_WORDS) rowmap[r - r0] = i | (g << 10) | (sm << 14) | (k << 16);
        }
      }
    }
    if (r0 == 0u && wave == 0u) {   // tile_row_off = the runs' look-back words (two dwords each); row_cursor[1] = total rows, written by the last run
#ifdef MKP_DEBUG
      uint32_t base;
      // ablation: no look-back (rows in completion order)
      if (prm.debug_skip & 4096u) { uint32_t b0 = 0; if (lane == 0) b0 = atomicAdd(row_cursor + 1, tile_rows);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0); }
      else base = lookback_reserve_wave(reinterpret_cast<unsigned long long*>(tile_row_off), run, tile_rows);
#else
      const uint32_t base = lookback_reserve_wave(reinterpret_cast<unsigned long long*>(tile_row_off), run, tile_rows);
#endif
      if (lane == 0) {
#ifdef MKP_DEBUG
        if (!(prm.debug_skip & 4096u))
#endif
        if (run + 1u == n_runs) row_cursor[1] = base + tile_rows;
        uint32_t s = tile_rows;
        if (base + s > prm.row_capacity) { atomicOr(dev_err, ERR_ROW_CAP); s = 0; }
        *row_base_p = base; *row_total_p = s;
      }
    }
    __syncthreads();
    // ---- E3: one thread per row
    const uint32_t n_here = rows_this_round(*row_total_p, r0, MKP_STREAM_ROWMAP_WORDS);
    for (uint32_t rr = threadIdx.x; rr < n_here; rr += PILEUP_THREADS) {
      const uint32_t e = rowmap[rr], si = e & 1023u, g = (e >> 10) & 15u, sm = (e >> 14) & 3u, k = (e >> 16) & 3u;
      const uint32_t ax = aux[si], combo = (ax & 0xffu) >> 2;
      RowAcc acc = {0, 0, 0, 0, 0, 0, 0, 0};
      uint32_t strand, motif1;   // motif1 = motif id + 1 (0: none)
      if (!combine) {
        stream_row_add<WIDE>(tal, S, P, sm, si, g, acc);
        strand = sm; motif1 = 0;
        if (combo) { const MkpCombo& cb = combos_l[combo]; const uint32_t n_ids = sm ? cb.n_neg : cb.n_pos;
          if (n_ids) motif1 = (uint32_t)(sm ? cb.neg_ids[k] : cb.pos_ids[k]) + 1u;
          }
      } else {
        const MkpCombo& cb = combos_l[combo];
        const uint32_t pd = (ax >> (8u + 6u * sm)) & 63u, iq = si + pd - 32u;
        const bool pos_ok = (ax & 1u) != 0, neg_ok = pd != 0u;
        for (uint32_t gj = g; gj < n_groups && (gj == g || !((P.info[gj] >> 18) & 1u)); gj++) {
          if (pos_ok && stream_row_exists<WIDE>(tal, S, n_counters, P, 0, si, gj)) stream_row_add<WIDE>(tal, S, P, 0, si, gj, acc);
          if (neg_ok && stream_row_exists<WIDE>(tal, S, n_counters, P, 1, iq, gj)) stream_row_add<WIDE>(tal, S, P, 1, iq, gj, acc);
        }
        strand = 2; motif1 = (uint32_t)cb.pos_ids[sm] + 1u;
      }
      store_row(rows, (size_t)*row_base_p + r0 + rr, (uint32_t)fpos[si], strand | (motif1 << 8) | (key << 16), P.code[g], acc);
    }
  }
}

// Rows of a pileup-hemi tile (the tail of mkp_pileup_tiles_hemi).  The host planner caps such a tile at one column per thread
// (MKP_PILEUP_THREADS): every thread counts its column's rows once, the block scans (column order = position order), thread 0
// reserves the tile's run of the row buffer with one atomic (mkp_scan_tiles + mkp_gather_rows order the runs afterwards), and the
// same threads write — position and count stay in registers.
__device__ __forceinline__ void emit_hemi_rows(const uint32_t* __restrict__ tal, SlotMap sm, uint32_t n_tslots, MkpTile tl, uint32_t run,
    const MkpRunParams& prm, uint32_t* __restrict__ rows_base, uint32_t* __restrict__ row_cursor, uint32_t* __restrict__ tile_row_off,
    uint32_t* __restrict__ tile_row_cnt, uint32_t* __restrict__ dev_err, uint32_t* wave_tot, uint32_t* row_base_p, uint32_t* row_total_p) {
  const MkpRowsDev rows = rows_view(rows_base, prm.row_capacity);
  const uint32_t i = threadIdx.x;
  uint32_t cnt = 0; int32_t p = 0;
  if (i < n_tslots) {
    p = sm.pos_of(i);
    if (p >= tl.r0 && p < tl.r1) cnt = hemi_rows_at<false>(tal, prm.slot_cap, prm, p, i, rows, 0);
  }
  uint32_t tile_rows;
  const uint32_t off = block_excl_scan(cnt, wave_tot, &tile_rows);
  if (threadIdx.x == 0) {
    uint32_t s = tile_rows;
    const uint32_t base = s ? atomicAdd(row_cursor, s) : 0u;
    if (base + s > prm.row_capacity) { atomicOr(dev_err, ERR_ROW_CAP); s = 0; }
    *row_base_p = base; *row_total_p = s; tile_row_off[run] = base; tile_row_cnt[run] = s;
  }
  __syncthreads();
  if (*row_total_p && cnt) hemi_rows_at<true>(tal, prm.slot_cap, prm, p, i, rows, *row_base_p + off);
}
