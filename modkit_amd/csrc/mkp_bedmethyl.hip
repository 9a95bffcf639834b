// The device bedMethyl reader: a piece of bedMethyl text in HBM — the output of the BGZF inflate kernel, or plain bytes uploaded as they are
// — becomes the eleven row columns of MkpRowsDev and the piece's contig runs.  The text and the rows never visit the host (host side:
// bedmethyl_in_* of mkp_api.cpp).  The grammar of a line is mkp_bedmethyl_parse_line (mkp_bedmethyl_line.hpp), the one the host reader runs.
//
// A data line is a line whose first byte is not '#'; byte 0 of the piece starts a line; a last line without '\n' counts when the piece is
// the file's last, otherwise it is the unfinished tail the host carries into the next piece.  Count / scan / write, as the ingest's chain
// kernels, five launches on the caller's stream around one host round trip (the row count sizes the row buffers):
//   mkp_bedmethyl_count    a workgroup per chunk of MKP_BEDIN_CHUNK bytes, a 16-byte load per lane: the data lines that start in the chunk,
//                          its '\n' count and the offset behind its last '\n', three words per chunk (no atomic)
//   mkp_bedmethyl_scan     one workgroup: exclusive scan of the data-line counts; the totals, the row count and the limit (where the last
//                          whole line ends) to the piece's words
//   [the host reads the words]
//   mkp_bedmethyl_starts   a workgroup per chunk again: the byte offset of every data line to line_start[], the limit behind the last
//   mkp_bedmethyl_parse    a lane per row: finds the line's end, parses, stores the eleven columns (column-major: coalesced 4-byte stores)
//   mkp_bedmethyl_runs     a lane per row: a row whose chrom bytes differ from the row before starts a run (one atomic per RUN appends it and
//                          its name; the host sorts the short list by row); inside a run pos must not descend
// A line is read straight from global memory, a byte at a time: the lanes of a wave hold 64 consecutive lines (about 5 KB of text), so a
// wave's loads fall into a few dozen cache lines that stay in the CU's L1 while the wave walks them.  Staging a workgroup's span in LDS was
// not done: the span of 256 lines has no bound ('#' lines and long lines lie between them), so the kernel would need this path anyway.
// Errors: bits in the error word and a 64-bit atomicMin of the offending line's offset, touched only when something is wrong.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkp_bedmethyl_line.hpp"
#include "mkp_launch.h"

namespace {

constexpr uint32_t kChunk = MKP_BEDIN_CHUNK, kThreads = 256, kPerLane = kChunk / kThreads;
static_assert(kPerLane == 16, "a lane reads one 16-byte vector");

struct ColsOut { uint32_t* c[11]; };     // pos, info, code, n_valid, n_mod, n_can, n_other, n_del, n_fail, n_diff, n_nocall

// the lane's 16 bytes at `off` (a multiple of 16; the buffer is padded to whole chunks) and the byte in front of them ('\n' in front of byte 0)
struct LaneBytes { uint32_t w[4]; uint8_t prev; };
__device__ __forceinline__ LaneBytes lane_bytes(const uint8_t* __restrict__ text, uint32_t off) {
  LaneBytes b;
  const uint4 v = *reinterpret_cast<const uint4*>(text + off);
  b.w[0] = v.x; b.w[1] = v.y; b.w[2] = v.z; b.w[3] = v.w;
  b.prev = off ? text[off - 1u] : (uint8_t)'\n';
  return b;
}
__device__ __forceinline__ uint8_t byte_of(const LaneBytes& b, uint32_t j) { return (uint8_t)(b.w[j >> 2] >> (8u * (j & 3u))); }
// data lines that start in the lane's bytes (those in front of n)
__device__ __forceinline__ uint32_t lane_starts(const LaneBytes& b, uint32_t off, uint32_t n) {
  uint32_t k = 0; uint8_t prev = b.prev;
#pragma unroll
  for (uint32_t j = 0; j < kPerLane; j++) { const uint8_t c = byte_of(b, j); k += (off + j < n && prev == '\n' && c != '#') ? 1u : 0u; prev = c; }
  return k;
}

__global__ __launch_bounds__(256) void mkp_bedmethyl_count(const uint8_t* __restrict__ text, uint32_t n, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_data[4], s_nl[4], s_last[4];
  const uint32_t t = threadIdx.x, off = blockIdx.x * kChunk + t * kPerLane;
  uint32_t data = 0, nl = 0, last = 0;
  if (off < n) {
    const LaneBytes b = lane_bytes(text, off);
    data = lane_starts(b, off, n);
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; j++) if (off + j < n && byte_of(b, j) == '\n') { nl++; last = off + j + 1u; }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    data += (uint32_t)__shfl_xor((int)data, d); nl += (uint32_t)__shfl_xor((int)nl, d);
    const uint32_t o = (uint32_t)__shfl_xor((int)last, d); last = o > last ? o : last;
  }
  if ((t & 63u) == 0u) { s_data[t >> 6] = data; s_nl[t >> 6] = nl; s_last[t >> 6] = last; }
  __syncthreads();
  if (t == 0) {   // the chunk's three words: data lines, line ends, the offset behind the last line end (0: none)
    const uint32_t n_chunks = gridDim.x;
    uint32_t m = s_last[0]; for (int k = 1; k < 4; k++) m = s_last[k] > m ? s_last[k] : m;
    cnt[blockIdx.x] = s_data[0] + s_data[1] + s_data[2] + s_data[3];
    cnt[n_chunks + blockIdx.x] = s_nl[0] + s_nl[1] + s_nl[2] + s_nl[3];
    cnt[2u * n_chunks + blockIdx.x] = m;
  }
}

// cnt[0, n_chunks) -> its exclusive scan, in place; the chunks' line ends summed and the last one found; the piece's totals to its words
__global__ __launch_bounds__(1024) void mkp_bedmethyl_scan(const uint8_t* __restrict__ text, uint32_t n, uint32_t final_piece, uint32_t* __restrict__ cnt,
    uint32_t n_chunks, uint32_t* __restrict__ words) {
  __shared__ uint32_t s[1024];
  __shared__ uint32_t s_nl, s_last;
  const uint32_t t = threadIdx.x;
  if (t == 0) { s_nl = 0; s_last = 0; }
  uint32_t carry = 0, nl = 0, last = 0;
  for (uint32_t base = 0; base < n_chunks; base += 1024u) {
    const uint32_t k = base + t, v = k < n_chunks ? cnt[k] : 0u;
    if (k < n_chunks) { nl += cnt[n_chunks + k]; const uint32_t o = cnt[2u * n_chunks + k]; last = o > last ? o : last; }
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
      const uint32_t add = t >= d ? s[t - d] : 0u;
      __syncthreads();
      s[t] += add;
      __syncthreads();
    }
    if (k < n_chunks) cnt[k] = carry + s[t] - v;
    carry += s[1023];
    __syncthreads();
  }
  if (nl) { atomicAdd(&s_nl, nl); atomicMax(&s_last, last); }   // (LDS)
  __syncthreads();
  if (t == 0) {
    const uint32_t limit = final_piece ? n : s_last;
    // the unfinished line behind the limit was counted when it is a data line
    const uint32_t tail = (limit < n && text[limit] != '#') ? 1u : 0u;
    words[MKP_BEDIN_W_LINES] = carry; words[MKP_BEDIN_W_ROWS] = carry - tail; words[MKP_BEDIN_W_LIMIT] = limit;
    words[MKP_BEDIN_W_NL] = s_nl; words[MKP_BEDIN_W_LAST_NL] = s_last;
  }
}

// line_start[k] = the offset of data line k, k < n_lines; line_start[n_rows] = limit (n_rows = n_lines, or n_lines - 1: the unfinished line
// starts at the limit)
__global__ __launch_bounds__(256) void mkp_bedmethyl_starts(const uint8_t* __restrict__ text, uint32_t n, const uint32_t* __restrict__ chunk_off,
    uint32_t n_rows, uint32_t limit, uint32_t* __restrict__ line_start) {
  __shared__ uint32_t s_wave[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, off = blockIdx.x * kChunk + t * kPerLane;
  LaneBytes b; b.w[0] = b.w[1] = b.w[2] = b.w[3] = 0; b.prev = 0;
  uint32_t mine = 0;
  if (off < n) { b = lane_bytes(text, off); mine = lane_starts(b, off, n); }
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d); if (lane >= (uint32_t)d) incl += o; }
  if (lane == 63u) s_wave[t >> 6] = incl;
  __syncthreads();
  uint32_t at = chunk_off[blockIdx.x] + incl - mine;
  for (uint32_t w = 0; w < (t >> 6); w++) at += s_wave[w];
  if (mine) {
    uint8_t prev = b.prev;
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; j++) { const uint8_t c = byte_of(b, j);
      if (off + j < n && prev == '\n' && c != '#') line_start[at++] = off + j;
      prev = c; }
  }
  if (blockIdx.x == 0 && t == 0) line_start[n_rows] = limit;
}

__global__ __launch_bounds__(256) void mkp_bedmethyl_parse(const uint8_t* __restrict__ text, const uint32_t* __restrict__ line_start, uint32_t n_rows,
    uint32_t max_line, ColsOut out, uint32_t* __restrict__ words) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_rows) return;
  const uint32_t limit = line_start[n_rows], s = line_start[i];
  uint32_t e = s;
  while (e < limit && text[e] != '\n') e++;
  MkpBedLine L;
  const uint32_t code = mkp_bedmethyl_parse_line(text + s, e - s, &L);
  uint32_t bits = !code ? 0u : MKP_BML_CLASS(code) == MKP_BML_BEYOND_32 ? MKP_BEDIN_ERR_RANGE : MKP_BEDIN_ERR_PARSE;
  if (e - s > max_line) bits |= MKP_BEDIN_ERR_LONG;
  if (bits) {
    atomicOr(&words[MKP_BEDIN_W_ERR], bits);
    atomicMin(reinterpret_cast<unsigned long long*>(words + MKP_BEDIN_W_ERR_OFF), (unsigned long long)s);
    L.pos = L.code = L.strand = L.n_valid = L.n_mod = L.n_canonical = L.n_other = L.n_delete = L.n_fail = L.n_diff = L.n_nocall = 0u;
  }
  out.c[0][i] = L.pos; out.c[1][i] = L.strand; out.c[2][i] = L.code; out.c[3][i] = L.n_valid; out.c[4][i] = L.n_mod; out.c[5][i] = L.n_canonical;
  out.c[6][i] = L.n_other; out.c[7][i] = L.n_delete; out.c[8][i] = L.n_fail; out.c[9][i] = L.n_diff; out.c[10][i] = L.n_nocall;
}

// the chrom of the line at s: its first field, [*cs, *cs + *cl)
__device__ __forceinline__ void chrom_of(const uint8_t* __restrict__ text, uint32_t s, uint32_t limit, uint32_t* cs, uint32_t* cl) {
  uint32_t p = s;
  while (p < limit && mkp_bml_sep(text[p])) p++;
  *cs = p;
  while (p < limit && !mkp_bml_sep(text[p]) && text[p] != '\n') p++;
  *cl = p - *cs;
}

__global__ __launch_bounds__(256) void mkp_bedmethyl_runs(const uint8_t* __restrict__ text, const uint32_t* __restrict__ line_start, uint32_t n_rows,
    const uint32_t* __restrict__ pos, MkpBedRun* __restrict__ runs, uint8_t* __restrict__ names, uint32_t* __restrict__ words) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_rows) return;
  const uint32_t limit = line_start[n_rows], s = line_start[i];
  uint32_t cs, cl; chrom_of(text, s, limit, &cs, &cl);
  bool head = i == 0u;
  if (i) {
    uint32_t ps, pl; chrom_of(text, line_start[i - 1u], limit, &ps, &pl);
    head = pl != cl;
    for (uint32_t k = 0; k < cl && !head; k++) head = text[ps + k] != text[cs + k];
    if (!head && pos[i] < pos[i - 1u]) {
      atomicOr(&words[MKP_BEDIN_W_ERR], MKP_BEDIN_ERR_ORDER);
      atomicMin(reinterpret_cast<unsigned long long*>(words + MKP_BEDIN_W_ERR_OFF), (unsigned long long)s);
    }
  }
  if (head) {
    const uint32_t k = atomicAdd(&words[MKP_BEDIN_W_RUNS], 1u), o = atomicAdd(&words[MKP_BEDIN_W_NAME_BYTES], cl);
    runs[k] = {i, o, cl};
    for (uint32_t j = 0; j < cl; j++) names[o + j] = text[cs + j];
  }
  if (i == 0u) words[MKP_BEDIN_W_FIRST_POS] = pos[0];
  if (i == n_rows - 1u) words[MKP_BEDIN_W_LAST_POS] = pos[i];
}

}  // namespace

extern "C" uint32_t mkp_bedmethyl_chunk_bytes(void) { return kChunk; }

// host-side entry points (declared in mkp_launch.h)

// text[0, n) (the buffer reaches to the next multiple of MKP_BEDIN_CHUNK), n > 0; cnt: three words per chunk; words: zeroed, ERR_OFF all ones
extern "C" hipError_t mkp_launch_bedmethyl_lines(hipStream_t st, const uint8_t* text, uint32_t n, uint32_t final_piece, uint32_t* cnt, uint32_t* words) {
  if (!n) return hipErrorInvalidValue;
  const uint32_t n_chunks = (n + kChunk - 1u) / kChunk;
  mkp_bedmethyl_count<<<n_chunks, kThreads, 0, st>>>(text, n, cnt);
  mkp_bedmethyl_scan<<<1, 1024, 0, st>>>(text, n, final_piece, cnt, n_chunks, words);
  return hipGetLastError();
}

// n_lines / n_rows / limit: the words as mkp_launch_bedmethyl_lines left them; chunk_off: its cnt; line_start: n_lines + 1 words; rows: n_rows
// rows a column; runs: n_rows entries; names: n bytes; max_line: the longest line (without its '\n') that is not MKP_BEDIN_ERR_LONG
extern "C" hipError_t mkp_launch_bedmethyl_parse(hipStream_t st, const uint8_t* text, uint32_t n, uint32_t n_lines, uint32_t n_rows, uint32_t limit,
    uint32_t max_line, const uint32_t* chunk_off, uint32_t* line_start, const MkpRowsDev* rows, MkpBedRun* runs, uint8_t* names, uint32_t* words) {
  if (!n || n_rows > n_lines || limit > n) return hipErrorInvalidValue;
  const uint32_t n_chunks = (n + kChunk - 1u) / kChunk;
  mkp_bedmethyl_starts<<<n_chunks, kThreads, 0, st>>>(text, n, chunk_off, n_rows, limit, line_start);
  if (n_rows) {
    const ColsOut out = {{rows->pos, rows->info, rows->code, rows->n_valid, rows->n_mod, rows->n_can, rows->n_other, rows->n_del, rows->n_fail,
        rows->n_diff, rows->n_nocall}};
    const uint32_t blocks = (n_rows + kThreads - 1u) / kThreads;
    mkp_bedmethyl_parse<<<blocks, kThreads, 0, st>>>(text, line_start, n_rows, max_line, out, words);
    mkp_bedmethyl_runs<<<blocks, kThreads, 0, st>>>(text, line_start, n_rows, rows->pos, runs, names, words);
  }
  return hipGetLastError();
}
