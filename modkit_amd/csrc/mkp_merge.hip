// `modkit bedmethyl merge` (merge_data, src/bedmethyl_util/subcommands.rs:136-195) over bedMethyl rows in HBM: an outer join of row sets on
// (start, mod code, strand) that sums the eight count columns, ordered by start, then strand ('+' < '-' < '.': StrandRule, src/util.rs:297-307),
// then code.  The sort calls Ord::cmp on the code (subcommands.rs:186), and ModCodeRepr DERIVES Ord (src/mod_base_code.rs:105-109: Code(char)
// before ChEbi(u32), letters by code point, numbers by number); its hand-written PartialOrd (141-150), which puts ChEBI numbers first, is not
// what `cmp` runs.  That is the numeric order of code_repr (a ChEBI number carries bit 31), the order the pileup's own rows come in.
//
// The primitive: A (the contig's merged table so far: ordered by the key, keys distinct) and B (the rows being added: ascending in `pos`, in any
// order inside a position, keys may repeat) give a new A.  The reference puts every line of every input into one map, so two rows of ONE input
// that share a key are summed too (the rows of a multi-motif run at one position): a run of equal keys may be longer than two, and the add
// into an empty A still runs everything.
//
// The key is pos (32 bits), strand rank (2) and code (32): 66 bits, compared as two words — {pos << 2 | rank} in 64 bits and code_repr as
// it is — so there is no code table and no cap on distinct codes.
//
// Four launches on the caller's stream, no host round trip between them:
//   mkp_merge_partition  one thread per tile boundary: the merge-path split of diagonal k * MKP_MERGE_TILE by `pos`, then moved back to the
//                        start of the position it lands in, in both inputs.  Every cut is a position boundary, so a run of equal keys is
//                        never split; a tile holds at most MKP_MERGE_TILE rows plus what one position holds.
//   mkp_merge_tile       a workgroup per tile: the two slices' keys and source indices into LDS, a bitonic sort by key, run heads by ballot,
//                        a block scan of the heads; the lane of a head walks its run (short: a position holds few rows per key) and sums
//                        the eight counters in 64 bits from HBM.  A sum beyond 2^32 - 1 sets MKP_MERGE_ERR_SUM and stores 2^32 - 1, never a
//                        wrapped value.  The tile's rows go to a staging table at the tile's INPUT offset (its output is no longer), its
//                        row count to counts[tile].  A tile with more than MKP_MERGE_CAP rows (one position with more than
//                        MKP_MERGE_CAP - MKP_MERGE_TILE rows) sets MKP_MERGE_ERR_TILE and writes nothing.
//   mkp_merge_scan       one workgroup: exclusive scan of the tile counts, the total to *n_out.
//   mkp_merge_compact    a workgroup per tile copies its staged rows to their place in the new table, all eleven columns, coalesced.
// No global atomic per row (the error word is touched only when something is wrong), vector stores only.
#include "mkp_dev_codeslots.hpp"
#include "mkp_launch.h"

namespace {

constexpr uint32_t kStep = MKP_MERGE_TILE, kCap = MKP_MERGE_CAP, kThreads = 256;
static_assert((kCap & (kCap - 1u)) == 0 && kCap % kThreads == 0 && kStep < kCap, "the LDS sort works on powers of two");

struct Cols { const uint32_t* c[11]; };     // pos, info, code, n_valid, n_mod, n_can, n_other, n_del, n_fail, n_diff, n_nocall
struct ColsOut { uint32_t* c[11]; };

__device__ __forceinline__ uint32_t pos_at(const uint32_t* __restrict__ a, uint32_t n, uint32_t i) { return i < n ? a[i] : 0xffffffffu; }

// cuts[k] = {rows of A, rows of B} in front of tile k; cuts[n_tiles] = {n_a, n_b}
__global__ __launch_bounds__(256) void mkp_merge_partition(const uint32_t* __restrict__ pos_a, uint32_t n_a, const uint32_t* __restrict__ pos_b,
    uint32_t n_b, uint32_t n_tiles, MkpMergeCut* __restrict__ cuts) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_tiles) return;
  const unsigned long long total = (unsigned long long)n_a + n_b, d64 = (unsigned long long)k * kStep;
  if (d64 >= total) { cuts[k] = {n_a, n_b}; return; }
  const uint32_t d = (uint32_t)d64;
  // the merge path by `pos` (A first among equals): the least a with pos_a[a] > pos_b[d - a - 1]
  uint32_t lo = d > n_b ? d - n_b : 0u, hi = d < n_a ? d : n_a;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (pos_a[mid] <= pos_b[d - mid - 1u]) lo = mid + 1u; else hi = mid;
  }
  const uint32_t a = lo, b = d - lo;
  const uint32_t pa = pos_at(pos_a, n_a, a), pb = pos_at(pos_b, n_b, b), p = pa < pb ? pa : pb;   // (a + b < total: one of the two exists)
  cuts[k] = {lower_bound_u32(pos_a, a, p), lower_bound_u32(pos_b, b, p)};
}

__global__ __launch_bounds__(256) void mkp_merge_tile(Cols A, Cols B, const MkpMergeCut* __restrict__ cuts, ColsOut stage, uint32_t* __restrict__ counts,
    uint32_t* err) {
  __shared__ unsigned long long s_key[kCap];   // pos << 2 | strand rank
  __shared__ uint32_t s_code[kCap];            // code_repr
  __shared__ uint32_t s_src[kCap];             // row of A, or row of B | 1 << 31
  __shared__ uint32_t s_wave[kThreads / 64];
  const uint32_t t = threadIdx.x, tile = blockIdx.x;
  const MkpMergeCut c0 = cuts[tile], c1 = cuts[tile + 1u];
  const uint32_t na = c1.a - c0.a, nb = c1.b - c0.b;
  const unsigned long long n64 = (unsigned long long)na + nb;
  if (n64 > kCap) {   // (block-uniform)
    if (t == 0) { atomicOr(err, MKP_MERGE_ERR_TILE); counts[tile] = 0u; }
    return;
  }
  const uint32_t n = (uint32_t)n64;
  if (n == 0u) { if (t == 0) counts[tile] = 0u; return; }
  uint32_t m = 64u; while (m < n) m <<= 1;   // the sort's size: a power of two, at most kCap
  for (uint32_t i = t; i < m; i += kThreads) {
    unsigned long long key = ~0ull; uint32_t code = 0xffffffffu, src = 0u;
    if (i < n) {
      const bool from_b = i >= na;
      const uint32_t r = from_b ? c0.b + (i - na) : c0.a + i;
      const Cols& S = from_b ? B : A;
      key = ((unsigned long long)S.c[0][r] << 2) | (S.c[1][r] & 3u);   // info: 0 '+', 1 '-', 2 '.' in its low bits, the rank itself
      code = S.c[2][r];
      src = r | (from_b ? 0x80000000u : 0u);
    }
    s_key[i] = key; s_code[i] = code; s_src[i] = src;
  }
  __syncthreads();
  // bitonic sort of m entries by (key, code); entries of one key end up next to each other in any order
  for (uint32_t size = 2u; size <= m; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
      for (uint32_t j = t; j < (m >> 1); j += kThreads) {
        const uint32_t i = 2u * j - (j & (stride - 1u)), p = i + stride;   // i has bit `stride` clear
        const bool up = (i & size) == 0u;
        const unsigned long long ki = s_key[i], kp = s_key[p]; const uint32_t ci = s_code[i], cp = s_code[p];
        const bool gt = ki > kp || (ki == kp && ci > cp);
        if (gt == up) { s_key[i] = kp; s_key[p] = ki; s_code[i] = cp; s_code[p] = ci; const uint32_t x = s_src[i]; s_src[i] = s_src[p]; s_src[p] = x; }
      }
      __syncthreads();
    }
  }
  // run heads, 256 entries a round: ballot inside a wave, the waves' totals through LDS
  const uint32_t base = c0.a + c0.b;   // the tile's place in the staging table: its input offset
  const int lane = lane_id(); const uint32_t wave = t >> 6;
  uint32_t done = 0u;
  for (uint32_t i0 = 0u; i0 < m; i0 += kThreads) {   // (block-uniform trip count)
    const uint32_t i = i0 + t;
    const bool head = i < n && (i == 0u || s_key[i] != s_key[i - 1u] || s_code[i] != s_code[i - 1u]);
    const unsigned long long heads = __ballot(head);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(heads);
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kThreads / 64; w++) { const uint32_t v = s_wave[w]; all += v; if (w < wave) before += v; }
    if (head) {
      const unsigned long long key = s_key[i]; const uint32_t code = s_code[i];
      unsigned long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (uint32_t j = i; j < n && s_key[j] == key && s_code[j] == code; j++) {
        const uint32_t src = s_src[j], r = src & 0x7fffffffu;
        const Cols& S = (src >> 31) ? B : A;
#pragma unroll
        for (int k = 0; k < 8; k++) sum[k] += S.c[3 + k][r];
      }
      const uint32_t o = base + done + before + (uint32_t)__popcll(heads & lanemask_lt());
      stage.c[0][o] = (uint32_t)(key >> 2); stage.c[1][o] = (uint32_t)(key & 3ull);   // the motif of a resident row does not survive
      stage.c[2][o] = code;
      bool over = false;
#pragma unroll
      for (int k = 0; k < 8; k++) { over = over || sum[k] > 0xffffffffull; stage.c[3 + k][o] = sum[k] > 0xffffffffull ? 0xffffffffu : (uint32_t)sum[k]; }
      if (over) atomicOr(err, MKP_MERGE_ERR_SUM);
    }
    done += all;
    __syncthreads();   // s_wave is rewritten by the next round
  }
  if (t == 0) counts[tile] = done;
}

// offsets[k] = rows in front of tile k in the new table; *n_out = all of them
__global__ __launch_bounds__(1024) void mkp_merge_scan(const uint32_t* __restrict__ counts, uint32_t n_tiles, uint32_t* __restrict__ offsets,
    uint32_t* __restrict__ n_out) {
  __shared__ uint32_t s[1024];
  const uint32_t t = threadIdx.x;
  uint32_t carry = 0u;
  for (uint32_t k0 = 0u; k0 < n_tiles; k0 += 1024u) {   // (block-uniform)
    const uint32_t k = k0 + t, v = k < n_tiles ? counts[k] : 0u;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {
      const uint32_t add = t >= d ? s[t - d] : 0u;
      __syncthreads();
      s[t] += add;
      __syncthreads();
    }
    if (k < n_tiles) offsets[k] = carry + s[t] - v;
    carry += s[1023];
    __syncthreads();
  }
  if (t == 0) *n_out = carry;
}

__global__ __launch_bounds__(256) void mkp_merge_compact(ColsOut stage, const MkpMergeCut* __restrict__ cuts, const uint32_t* __restrict__ counts,
    const uint32_t* __restrict__ offsets, ColsOut out) {
  const uint32_t tile = blockIdx.x, n = counts[tile];
  const MkpMergeCut c0 = cuts[tile];
  const uint32_t from = c0.a + c0.b, to = offsets[tile];
  for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
#pragma unroll
    for (int k = 0; k < 11; k++) out.c[k][to + i] = stage.c[k][from + i];
  }
}

// the rows in front of `limit` of an ascending `pos` column (rows at pos >= the contig's length are dropped by the caller)
__global__ void mkp_merge_rows_below(const uint32_t* __restrict__ pos, uint32_t n, uint32_t limit, uint32_t* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = lower_bound_u32(pos, n, limit);
}

Cols cols_of(const MkpRowsDev& r) {
  return {{r.pos, r.info, r.code, r.n_valid, r.n_mod, r.n_can, r.n_other, r.n_del, r.n_fail, r.n_diff, r.n_nocall}};
}
ColsOut cols_out_of(const MkpRowsDev& r) {
  return {{r.pos, r.info, r.code, r.n_valid, r.n_mod, r.n_can, r.n_other, r.n_del, r.n_fail, r.n_diff, r.n_nocall}};
}

}  // namespace

extern "C" uint32_t mkp_merge_tile_rows(void) { return kStep; }

// host-side entry points (declared in mkp_launch.h)
extern "C" uint32_t mkp_merge_tiles(uint64_t n_rows) { return (uint32_t)((n_rows + kStep - 1u) / kStep); }

extern "C" hipError_t mkp_launch_merge_rows_below(hipStream_t st, const uint32_t* pos, uint32_t n, uint32_t limit, uint32_t* out) {
  mkp_merge_rows_below<<<1, 64, 0, st>>>(pos, n, limit, out);
  return hipGetLastError();
}

// a (n_a rows, by key, keys distinct) and b (n_b rows, ascending pos) -> out (capacity n_a + n_b rows), *n_out rows; stage: capacity
// n_a + n_b rows; cuts: mkp_merge_tiles(n_a + n_b) + 1 entries, counts / offsets: mkp_merge_tiles(n_a + n_b) each.
// ev (may be NULL): three events recorded in front of the partition kernel, in front of the tile kernel and behind the compaction
extern "C" hipError_t mkp_launch_merge(hipStream_t st, const MkpRowsDev* a, uint32_t n_a, const MkpRowsDev* b, uint32_t n_b, const MkpRowsDev* stage,
    const MkpRowsDev* out, MkpMergeCut* cuts, uint32_t* counts, uint32_t* offsets, uint32_t* n_out, uint32_t* err, hipEvent_t* ev) {
  const uint64_t total = (uint64_t)n_a + n_b;
  if (total > 0xffffffffull) return hipErrorInvalidValue;
  const uint32_t n_tiles = mkp_merge_tiles(total);
  hipError_t e;
  if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return e;
  if (!n_tiles) { if ((e = hipMemsetAsync(n_out, 0, 4, st)) != hipSuccess) return e; }
  else mkp_merge_partition<<<(n_tiles + 1u + 255u) / 256u, 256, 0, st>>>(a->pos, n_a, b->pos, n_b, n_tiles, cuts);
  if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return e;
  if (n_tiles) {
    mkp_merge_tile<<<n_tiles, kThreads, 0, st>>>(cols_of(*a), cols_of(*b), cuts, cols_out_of(*stage), counts, err);
    mkp_merge_scan<<<1, 1024, 0, st>>>(counts, n_tiles, offsets, n_out);
    mkp_merge_compact<<<n_tiles, kThreads, 0, st>>>(cols_out_of(*stage), cuts, counts, offsets, cols_out_of(*out));
  }
  if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return e;
  return hipGetLastError();
}
