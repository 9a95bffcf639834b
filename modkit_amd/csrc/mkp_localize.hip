// Localize (`modkit localize`, src/localise/util.rs:25-46, 189-227) over bedMethyl rows that are already in HBM: per mod code and offset
// from the anchor of a feature's window, n_mod = sum of N_mod, n_valid = sum of N_valid_cov and the number of rows, over every window
// [ws, we) and every row inside it whose strand passes the fetch rule (and the same / opposite test against the region's own strand).
//
// Input: the SoA row columns of one piece of one contig, ascending in `pos`, and the windows of that contig (any order, overlapping,
// repeating).  Every window adds into the SAME 2 w + 1 offsets, so a global atomic per row would queue thirty thousand windows on a few
// thousand addresses; the histogram is privatised in LDS instead.  Two launches on the caller's stream, no host round trip between them:
//   mkp_localize_bounds   one thread per window: lower_bound(ws) / lower_bound(we) in `pos`
//   mkp_localize_reduce   a workgroup owns one TILE of MKP_LOC_TILE offsets (blockIdx.x) and keeps [MKP_LOC_LOCAL slots][tile] cells of
//                         {n_mod, n_valid, n_rows} in LDS; blockIdx.y strides over batches of 256 windows.  Per batch: each thread finds the
//                         rows of one window that fall into the tile (two searches inside the window's range), the block scans the
//                         counts, then the threads sweep the flattened rows one row per thread, finding a row's window by a search in
//                         the scanned counts — work is balanced over rows, not windows.  The LDS cells are the LOW 32 bits of the sums,
//                         updated with returning LDS atomics; an add that wraps carries 1 << 32 into the HBM cell at once, so totals are
//                         exact in 64 bits at 12 bytes a cell.  At the end the workgroup adds its non-zero cells to the HBM table with
//                         contiguous 64-bit atomics.
// The table tab[slot][2 w + 1][3] lives for the whole run: pieces (shards) add into it, so a window across a seam counts each row once.
// Code slots are claimed by resolve_slot of mkp_dev_codeslots.hpp, shared with mkp_stats.hip (the first counted row of a code, one lane per
// wave and code); a code whose slot is beyond the LDS ones adds to HBM per row (rare, exact); a seventeenth code sets the error bit.
#include "mkp_dev_codeslots.hpp"
#include "mkp_launch.h"

namespace {

constexpr uint32_t kTile = MKP_LOC_TILE, kBatch = MKP_LOC_BATCH;
constexpr int kLocal = MKP_LOC_LOCAL;
constexpr uint32_t kCells = (uint32_t)kLocal * kTile * 3u;

__global__ __launch_bounds__(256) void mkp_localize_bounds(const uint32_t* __restrict__ pos, uint32_t n_rows, const MkpLocRegion* __restrict__ regions,
    uint32_t n_regions, uint32_t* __restrict__ row_lo, uint32_t* __restrict__ row_hi) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_regions) return;
  const MkpLocRegion g = regions[r];
  uint32_t lo, hi;
  row_range(pos, n_rows, g.ws, g.we, &lo, &hi);
  row_lo[r] = lo; row_hi[r] = hi;
}

// StrandRule::overlaps (src/util.rs:310-318) on rules 1 '+', 2 '-', 3 both
__device__ __forceinline__ bool overlaps(uint32_t a, uint32_t b) { return a == 3u || b == 3u || a == b; }

__global__ __launch_bounds__(256) void mkp_localize_reduce(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ info,
    const uint32_t* __restrict__ code, const uint32_t* __restrict__ n_valid, const uint32_t* __restrict__ n_mod,
    const MkpLocRegion* __restrict__ regions, uint32_t n_regions, const uint32_t* __restrict__ row_lo, const uint32_t* __restrict__ row_hi,
    uint32_t window, uint32_t stranded /* 0 none, 1 same, 2 opposite */, unsigned long long* __restrict__ tab, uint32_t* codes, uint32_t* err) {
  __shared__ uint32_t cell[kCells];                 // [slot][offset in tile][n_mod, n_valid, n_rows], low words
  __shared__ unsigned long long scan[kBatch + 1];   // rows of the batch's windows in this tile, exclusive prefix; [kBatch] = all
  __shared__ uint32_t s_first[kBatch], s_top[kBatch], s_rules[kBatch];
  const uint32_t t = threadIdx.x, n_off = 2u * window + 1u, o0 = blockIdx.x * kTile;   // the tile holds the offset indices [o0, o0 + kTile)
  const int lane = lane_id();
  for (uint32_t i = t; i < kCells; i += kBatch) cell[i] = 0u;
  uint32_t ctab = load_codes(codes, lane);   // the code table as this wave last saw it
  const uint32_t n_batches = (n_regions + kBatch - 1u) / kBatch;
  for (uint32_t batch = blockIdx.y; batch < n_batches; batch += gridDim.y) {
    __syncthreads();   // the cells are zero / the sweep before this one has read its batch
    // offset index = anchor + window - pos; the tile's index 0 is the row at `top`, its last one the row at top - (kTile - 1)
    const uint32_t r = batch * kBatch + t;
    uint32_t first = 0, cnt = 0, top32 = 0, rules = 0;
    if (r < n_regions) {
      const MkpLocRegion g = regions[r];
      const uint32_t lo = row_lo[r], hi = row_hi[r];
      const long long top = (long long)g.anchor + (long long)window - (long long)o0;
      if (top >= 0 && hi > lo) {
        const long long low = top - (long long)(kTile - 1u);
        const uint32_t a = lo + lower_bound_u32(pos + lo, hi - lo, low > 0 ? (uint32_t)low : 0u);
        const uint32_t b = top >= 0xffffffffll ? hi : lo + lower_bound_u32(pos + lo, hi - lo, (uint32_t)top + 1u);
        first = a; cnt = b > a ? b - a : 0u;
      }
      top32 = (uint32_t)top; rules = g.rules;
    }
    s_first[t] = first; s_top[t] = top32; s_rules[t] = rules;
    scan[t + 1u] = cnt; if (t == 0u) scan[0] = 0ull;
    __syncthreads();
    for (uint32_t d = 1; d < kBatch; d <<= 1) {
      const unsigned long long add = t + 1u > d ? scan[t + 1u - d] : 0ull;
      __syncthreads();
      scan[t + 1u] += add;
      __syncthreads();
    }
    const unsigned long long total = scan[kBatch];
    for (unsigned long long j0 = 0; j0 < total; j0 += kBatch) {   // (block-uniform trip count: every lane of a wave reaches the ballots)
      const unsigned long long j = j0 + t;
      bool pass = false; uint32_t c = 0, nv = 0, nm = 0, o = 0;
      if (j < total) {
        uint32_t a = 0, b = kBatch;   // scan[a] <= j < scan[b]: windows without rows share their successor's prefix and are never found
        while (b - a > 1u) { const uint32_t mid = a + ((b - a) >> 1); if (scan[mid] <= j) a = mid; else b = mid; }
        const uint32_t i = s_first[a] + (uint32_t)(j - scan[a]), rl = s_rules[a];
        const uint32_t row_rule = (info[i] & 3u) + 1u;   // info: 0 '+', 1 '-', 2 '.'
        c = code[i]; nv = n_valid[i]; nm = n_mod[i];
        o = s_top[a] - pos[i];   // in [0, kTile) by the two searches
        pass = overlaps(row_rule, rl & 0xffu);
        if (stranded) pass = pass && (overlaps(rl >> 8, row_rule) == (stranded == 1u));
        pass = pass && o < kTile && o0 + o < n_off;
      }
      const int slot = resolve_slot(ctab, codes, err, pass, c, true, lane);
      if (slot >= 0) {
        unsigned long long* hbm = tab + ((size_t)slot * n_off + o0 + o) * 3u;
        const uint32_t v[3] = {nm, nv, 1u};
        if (slot < kLocal) {
          uint32_t* lds = &cell[((uint32_t)slot * kTile + o) * 3u];
#pragma unroll
          for (int k = 0; k < 3; k++) if (v[k]) {
            const uint32_t old = atomicAdd(&lds[k], v[k]);
            if (old + v[k] < old) atomicAdd(&hbm[k], 1ull << 32);   // the low word wrapped: the carry goes to HBM now
          }
        } else {
#pragma unroll
          for (int k = 0; k < 3; k++) if (v[k]) atomicAdd(&hbm[k], (unsigned long long)v[k]);
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = t; i < kCells; i += kBatch) {
    const uint32_t v = cell[i];
    const uint32_t s = i / (kTile * 3u), rem = i - s * (kTile * 3u);
    if (v && o0 + rem / 3u < n_off) atomicAdd(&tab[((size_t)s * n_off + o0) * 3u + rem], (unsigned long long)v);
  }
}

}  // namespace

extern "C" uint32_t mkp_localize_tile_offsets(void) { return kTile; }

// host-side launcher (declared in mkp_launch.h).  ev (may be NULL): three events recorded in front of the bounds kernel, in front of the reduce
// kernel and behind it
extern "C" hipError_t mkp_launch_localize(hipStream_t st, const uint32_t* pos, const uint32_t* info, const uint32_t* code, const uint32_t* n_valid,
    const uint32_t* n_mod, uint32_t n_rows, const MkpLocRegion* regions, uint32_t n_regions, uint32_t* row_lo, uint32_t* row_hi, uint32_t window,
    uint32_t stranded, unsigned long long* tab, uint32_t* codes, uint32_t* err, hipEvent_t* ev) {
  if (!n_rows || !n_regions) return hipSuccess;
  hipError_t e;
  if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return e;
  mkp_localize_bounds<<<(n_regions + 255u) / 256u, 256, 0, st>>>(pos, n_rows, regions, n_regions, row_lo, row_hi);
  if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return e;
  // a workgroup flushes up to its whole tile at the end, so fewer workgroups mean fewer flush atomics; but a workgroup's batches run one
  // after the other, and measured on 30 000 windows of 4 001 offsets about four workgroups per CU (0.078 ms) beat one per CU (0.165 ms):
  // up to 1024 in all, fewer when the piece or the batch list is short (profiles/localize_c3.txt)
  const uint32_t n_tiles = (2u * window + 1u + kTile - 1u) / kTile, n_batches = (n_regions + kBatch - 1u) / kBatch;
  const uint32_t groups = std::max(1u, std::min({n_batches, std::max(1u, 1024u / n_tiles), (n_rows + 2047u) / 2048u}));
  mkp_localize_reduce<<<dim3(n_tiles, groups), 256, 0, st>>>(pos, info, code, n_valid, n_mod, regions, n_regions, row_lo, row_hi, window, stranded,
      tab, codes, err);
  if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return e;
  return hipGetLastError();
}
