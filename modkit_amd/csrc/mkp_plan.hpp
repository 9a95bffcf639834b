// Internal (not installed): the shard planner of libmkpileup.  From the packed reads of a shard (ShardHost) it derives everything a pass
// needs (run parameters, decode classes, event slices, tiles, candidate reads per tile, owners of shared names, fused and cover lists, work
// records) as one ShardPlan.  Host only: no HIP header is read here, g++ compiles it with mkp_pack.hpp and mkp_device.h behind it.
// make_resident (mkp_api.cpp) runs the stages in the order they stand here, copies the plan's scalars into the context and uploads.
#pragma once
#include <atomic>
#include <chrono>
#include <climits>
#include <functional>
#include <map>
#include <mutex>
#include <vector>

#include "mkp_pack.hpp"

namespace mkp {

template <class F> void host_parallel(size_t n, size_t grain, F f) {   // f(lo, hi) over [0, n) in `grain`-sized pieces on the host pool
  const size_t pieces = (n + grain - 1) / grain;
  HostPool::get().parallel(pieces, [&](size_t i) { f(i * grain, std::min(n, (i + 1) * grain)); });
}

// MKP_TRACE_PLAN: the host's stages on stderr, each with the time since the last mark; `kernels`: the indented marks of a launch sequence
struct PlanTrace {
  bool on, kernels; std::chrono::steady_clock::time_point last;
  explicit PlanTrace(bool on_, bool kernels_ = false, std::chrono::steady_clock::time_point from = std::chrono::steady_clock::now())
      : on(on_), kernels(kernels_), last(from) {}
  static bool wanted() { return getenv("MKP_TRACE_PLAN") != nullptr; }
  void lap(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[mkpileup plan] %s%-*s %.2f ms\n", kernels ? "  kernels: " : "", kernels ? 20 : 28, what,
        std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};

// the planner's environment knobs, read once per plan
struct PlanKnobs {
  bool fused_off = false;          // MKP_FUSED=0: every read takes its class's event decoder
  bool has_stream_tile = false; uint32_t stream_tile = 0;   // MKP_STREAM_TILE: slots per tile of the slot pipeline (experiments)
  uint32_t debug_skip = 0;         // MKP_DEBUG_SKIP (MKP_DEBUG builds only)
  bool strand_slots_off = false;   // MKP_STRAND_SLOTS=0: every fused read decodes all of its slots, not only those of its own strand
  static PlanKnobs from_env() {
    PlanKnobs k;
    if (const char* e = getenv("MKP_FUSED")) k.fused_off = !strcmp(e, "0");
    if (const char* e = getenv("MKP_STRAND_SLOTS")) k.strand_slots_off = !strcmp(e, "0");
    if (const char* e = getenv("MKP_STREAM_TILE")) { k.has_stream_tile = true; k.stream_tile = (uint32_t)strtoul(e, nullptr, 10); }
#ifdef MKP_DEBUG
    if (const char* e = getenv("MKP_DEBUG_SKIP")) k.debug_skip = (uint32_t)strtoul(e, nullptr, 0);
#endif
    return k;
  }
};

// ids reordered by key(id) DESCENDING, equal keys keeping their order (what std::stable_sort with `>` gives): three 11-bit counting passes
// — the planner sorts a shard's 200 000 reads by length three times, and comparison sorts were a third of its time
template <class Key> void stable_sort_desc(std::vector<uint32_t>& ids, Key key) {
  const size_t n = ids.size(); if (n < 2) return;
  if (n < 2048) { std::stable_sort(ids.begin(), ids.end(), [&](uint32_t x, uint32_t y) { return key(x) > key(y); }); return; }
  std::vector<uint32_t> k(n), tmp(n), ktmp(n);
  for (size_t i = 0; i < n; i++) k[i] = ~key(ids[i]);   // ascending in the complement = descending in the key
  for (int pass = 0; pass < 3; pass++) {
    const int sh = 11 * pass; size_t cnt[2049] = {0};
    for (size_t i = 0; i < n; i++) cnt[((k[i] >> sh) & 2047u) + 1]++;
    bool trivial = false; for (size_t b = 1; b <= 2048; b++) if (cnt[b] == n) trivial = true;
    if (trivial) continue;
    for (size_t b = 0; b < 2048; b++) cnt[b + 1] += cnt[b];
    for (size_t i = 0; i < n; i++) { const size_t at = cnt[(k[i] >> sh) & 2047u]++; tmp[at] = ids[i]; ktmp[at] = k[i]; }
    ids.swap(tmp); k.swap(ktmp);
  }
}
inline void sort_u32(std::vector<uint32_t>& v) {   // ascending, three 11-bit counting passes
  const size_t n = v.size(); if (n < 4096) { std::sort(v.begin(), v.end()); return; }
  std::vector<uint32_t> tmp(n);
  for (int pass = 0; pass < 3; pass++) {
    const int sh = 11 * pass; const uint32_t mask = pass == 2 ? 1023u : 2047u; size_t cnt[2049] = {0};
    for (size_t i = 0; i < n; i++) cnt[((v[i] >> sh) & mask) + 1]++;
    for (size_t b = 0; b < 2048; b++) cnt[b + 1] += cnt[b];
    for (size_t i = 0; i < n; i++) tmp[cnt[(v[i] >> sh) & mask]++] = v[i];
    v.swap(tmp);
  }
}

// reads by decode kernel: [SPARSE one tag | SPARSE two tags | FAST one tag | FAST two tags | everything else].
// FAST = one (strand, base) group, no code listed twice, at most two tags.  SPARSE = FAST with explicit ('?') tags only and,
// for two tags, identical rank lists (`C+h?,d..;C+m?,d..` as basecallers write them): the calls are located per call, not per base.
// With `duplex` (never for the threshold sampler): [.. | duplex one tag per group | duplex two]: reads whose layout has two groups on
// different bases (`C+h?;C+m?;G-h?;G-m?`), every tag explicit and the tags of a group sharing one rank list; such a read is listed
// twice (bit 31 = its second group), each listing decoded by a SPARSE wave, and mkp_merge_duplex interleaves the two event lists.
inline void class_ids(const ShardHost& S, const LayoutTables& T, std::vector<uint32_t>* ids, uint32_t n_class[7], bool duplex) {
  auto class_of = [&](size_t i) -> int {
    const MkpReadHdr& h = S.hdr[i];
    auto same = [&](uint32_t t0, uint32_t t1) {
      const MkpTagRef &a = S.tagref[h.tag_off + t0], &b = S.tagref[h.tag_off + t1];
      // compared on the device while the lists were written (only neighbours are ever asked about)
      if (S.dev_packed) return t1 == t0 + 1 && b.pad != 0;
      return a.n == b.n && (a.n == 0 || memcmp(&S.ranks[a.rank_off], &S.ranks[b.rank_off], 4 * (size_t)a.n) == 0); };
    if ((h.flags & MKP_RF_BAD) || !h.n_tags || h.layout >= T.dev.size()) return 4;
    const MkpLayout& L = T.dev[h.layout];
    bool explicit_tags = true;
    for (uint32_t t = 0; t < h.n_tags; t++) if (L.tags[t].mode != 0) explicit_tags = false;
    if (duplex && L.fast == 2) {
      const uint32_t nA = L.pad;
      if (explicit_tags && (nA != 2 || same(0, 1)) && (h.n_tags - nA != 2 || same(nA, nA + 1))) return (nA == 1 && h.n_tags - nA == 1) ? 5 : 6;
      return 4;
    }
    if (L.fast == 1 && h.n_tags <= 2) {
      const bool sparse = explicit_tags && (h.n_tags == 1 || same(0, 1));
      return (sparse ? 0 : 2) + (int)(h.n_tags - 1);
    }
    return 4;
  };
  // classified on all cores (the rank-list comparisons touch every call of a two-tag read); then one list per class,
  // one wave decodes one read start to end: the longest reads are launched first so that they do not form the kernel's tail
  std::vector<uint8_t> cl(S.hdr.size());
  host_parallel(S.hdr.size(), 4096, [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) cl[i] = (uint8_t)class_of(i); });
  std::vector<uint32_t> cls[7];
  for (size_t i = 0; i < cl.size(); i++) cls[cl[i]].push_back((uint32_t)i);
  host_parallel(7, 1, [&](size_t lo, size_t hi) {
    for (size_t c = lo; c < hi; c++) stable_sort_desc(cls[c], [&](uint32_t x) { return S.hdr[x].l_seq; }); });
  ids->clear();
  for (int c = 0; c < 5; c++) { n_class[c] = (uint32_t)cls[c].size(); ids->insert(ids->end(), cls[c].begin(), cls[c].end()); }
  for (int c = 5; c < 7; c++) {
    n_class[c] = 2u * (uint32_t)cls[c].size();
    for (uint32_t r : cls[c]) { ids->push_back(r); ids->push_back(r | 0x80000000u); }
  }
}

// MkpFusedDesc of a layout whose tags form one explicit-mode group (decode class SPARSE): the walk of
// MultipleThresholdModCaller::call (threshold_mod_caller.rs:28-63) over a call's map, resolved from the layout's caller tables
inline MkpFusedDesc fused_desc(const MkpLayout& D) {
  MkpFusedDesc f; memset(&f, 0, sizeof(f));
  if (D.fast != 1 || D.n_tags == 0 || D.n_tags > 2) return f;
  const uint32_t b0 = D.tags[0].fb & 3u, sg0 = D.tags[0].neg & 1u;
  const MkpGroupDesc& G = D.groups[sg0 * 4 + b0];
  uint32_t hit = 0; for (uint32_t t = 0; t < D.n_tags; t++) hit |= 1u << (D.tagmap[t][b0] & 15u);
  const uint32_t pv = G.pat[hit < 20u ? hit : 0u], n_post = std::min<uint32_t>((pv >> 3) & 7u, MKP_KMAX);
  uint32_t ob = 0;
  for (uint32_t i = 0; i < n_post; i++) {
    const uint32_t kq = (pv >> (16 + 2 * i)) & 3u;
    ob |= 1u << ((G.slots >> (8 * kq)) & 0xffu);
    f.it_cid |= ((G.cids >> (8 * kq)) & 0xffu) << (8 * i); f.it_thr[i] = G.thr_mod[kq];
    for (uint32_t t = 0; t < D.n_tags; t++) for (uint32_t k = 0; k < D.tags[t].n_codes; k++)
      if (((D.tagmap[t][b0] >> (4 + 4 * k)) & 15u) == kq) f.it_src |= (t | (k << 1)) << (4 * i);
  }
  f.misc = b0 | (sg0 << 2) | (n_post << 3) | (MKP_G_CIDCAN(G.misc) << 8) | (ob << 16);
  f.nc = (uint32_t)D.tags[0].n_codes | ((D.n_tags > 1 ? (uint32_t)D.tags[1].n_codes : 0u) << 8);
  f.thr_can = G.thr_can;
  // the thresholds of the integer caller: least T with T / 2048 >= threshold (exact in double: a float times 2^11)
  auto i_of = [](float thr) -> int32_t {
    if (!(thr == thr)) return INT32_MAX;
    const double t = std::ceil((double)thr * 2048.0);
    return (int32_t)std::max(-1073741824.0, std::min(1073741824.0, t)); };
  for (uint32_t i = 0; i < MKP_KMAX; i++) f.i_thr[i] = i_of(f.it_thr[i]);
  f.i_can = i_of(f.thr_can);
  f.misc |= 1u << 6;
  const int x = MKP_G_COLL(G.misc); const uint32_t n_pre = pv & 7u;   // collapse_redistribute's inputs (only looked at in collapse runs)
  bool col_exact = true;
  for (uint32_t i = 0; i < n_pre && i < MKP_KMAX; i++) if ((int)((pv >> (8 + 2 * i)) & 3u) == x) {
    f.col = 1u; f.n_other = (float)n_pre;
    for (uint32_t t = 0; t < D.n_tags; t++) for (uint32_t k = 0; k < D.tags[t].n_codes; k++)
      if ((int)((D.tagmap[t][b0] >> (4 + 4 * k)) & 15u) == x) f.col |= (t | (k << 1)) << 1;
    // (a share over three codes is rounded: the f32 walk stays)
    if (n_pre == 1 || n_pre == 2 || n_pre == 4) f.col |= (n_pre == 1 ? 0u : n_pre == 2 ? 1u : 2u) << 5; else col_exact = false;
  }
  if (col_exact) f.misc |= 1u << 7;
  return f;
}

// htslib's pileup engine (bam_plp_push; `set_max_depth` = bam_plp_set_maxcnt, pileup/mod.rs:755-759) refuses a record when it starts
// where the last buffered record started and the buffer — the records that end at or behind that position, plus the list's tail node —
// holds more than max_depth entries (`iter->pos == b->core.pos && iter->mp->cnt > iter->maxcnt`); the first record of a start is always
// taken, so depth alone drops nothing.  Every interval of the reference's grid is a fetch with an iterator of its own over the records
// that overlap it.  Dropping per (record, interval) is not reproduced on the device; what is decided here, exactly, is whether ANY
// record would be dropped: an interval [a, e) and a start b shared by two or more of its records with
//     #{records of the interval: start <= b and end >= b}  >  max_depth        (end > a where b <= a: the fetch's own condition).
// If there is none, htslib keeps every record at any depth and the device result is exact.  The population is htslib's: every record
// passing BAM_DEF_MASK (kept reads and supplementary ones), by reference span (ref-skips included).
// Returns whether the shard needs the wide tallies: a column that may hold more than 65 535 records overflows the 16-bit strand halves
// of the packed ones.  No (counter, strand, column) tally exceeds its column's record count — a record adds at most one feature per
// tally strand at a position (a second feature at one base is the other mod strand's call, on the other tally strand), one observed-code
// mark per slot and strand, one deletion — so the column depth is the bound.  Decided whenever the shard holds more than 65 535 records,
// whatever max_depth says.  pileup-hemi has no wide kernel: such a shard is refused there.
inline bool depth_guard(const ShardHost& S, uint32_t max_depth, const std::vector<uint32_t>& iv_starts, bool hemi) {
  const size_t n = S.hdr.size() + S.extra_spans.size();
  constexpr size_t kNarrowDepth = 65535;
  if (n <= max_depth && n <= kNarrowDepth) return false;
  std::vector<std::pair<uint32_t, uint32_t>> sp; sp.reserve(n);   // (start, end), starts ascending (alignment starts and ends are non-negative)
  for (auto& h : S.hdr) sp.push_back({(uint32_t)h.ref_start, (uint32_t)std::max(h.ref_end, h.ref_start + 1)});
  for (auto& x : S.extra_spans) sp.push_back({(uint32_t)x.first, (uint32_t)std::max(x.second, x.first + 1)});
  if (!std::is_sorted(sp.begin(), sp.end(), [](auto& x, auto& y) { return x.first < y.first; }))
    std::stable_sort(sp.begin(), sp.end(), [](auto& x, auto& y) { return x.first < y.first; });
  std::vector<uint32_t> en;   // ends ascending (built on first use)
  auto sorted_ends = [&]() { if (en.size() != n) { en.resize(n); for (size_t i = 0; i < n; i++) en[i] = sp[i].second; sort_u32(en); } };
  bool wide = false;
  if (n > kNarrowDepth) {
    // O(n) upper bound first: the records over a column p start in (p - L, p], L = the longest span — the most starts in any L positions
    uint64_t L = 0; for (auto& x : sp) L = std::max<uint64_t>(L, x.second - x.first);
    size_t bound = 0;
    for (size_t i = 0, j = 0; i < n; i++) { while ((uint64_t)sp[j].first + L <= sp[i].first) j++; bound = std::max(bound, i - j + 1); }
    if (bound > kNarrowDepth) {   // the exact deepest column: a sweep over starts and ends
      sorted_ends();
      size_t j = 0, cur = 0, best = 0;
      for (size_t i = 0; i < n; i++) { while (j < n && en[j] <= sp[i].first) { j++; cur--; } cur++; best = std::max(best, cur); }
      wide = best > kNarrowDepth;
    }
    if (wide && hemi) throw Error(MKP_E_UNSUPPORTED,
        "more than 65535 reads over one position: pileup-hemi columns this deep are outside the device path (16-bit packed tallies)");
  }
  if (n <= max_depth) return wide;
  sorted_ends();
  auto refuse = [&](uint32_t b, size_t held) {
    throw Error(MKP_E_UNSUPPORTED, "htslib would drop records here: " + std::to_string(held) + " buffered records at position " + std::to_string(b) +
        ", where several records start, exceed max_depth (" + std::to_string(max_depth) + "); bam_plp_push's maxcnt read dropping is not reproduced"); };
  auto ends_below = [&](uint32_t v) { return (size_t)(std::lower_bound(en.begin(), en.end(), v) - en.begin()); };   // #{end < v}
  // interval starts of the shard (none given: the shard is one interval)
  std::vector<uint32_t> A; A.push_back((uint32_t)std::max(S.win_start, 0));
  for (size_t k = 1; k < iv_starts.size(); k++) if (iv_starts[k] > A.back()) A.push_back(iv_starts[k]);
  // (1) starts b inside an interval (a <= b): the interval's fetch holds every record with start <= b <= end
  for (size_t i = 0; i < n;) {
    size_t r = i; while (r < n && sp[r].first == sp[i].first) r++;
    const uint32_t b = sp[i].first;
    if (r - i >= 2 && b >= A[0]) {
      const bool on_start = std::binary_search(A.begin(), A.end(), b);   // b == a: records that end AT a are not fetched
      const size_t held = r - (on_start ? ends_below(b + 1) : ends_below(b));
      if (held > max_depth) refuse(b, held);
    }
    i = r;
  }
  // (2) starts in front of an interval's start a: among the records with start < a < end
  for (uint32_t a : A) {
    const size_t before = (size_t)(std::lower_bound(sp.begin(), sp.end(), a, [](auto& x, uint32_t v) { return x.first < v; }) - sp.begin());
    if (before - std::min(before, ends_below(a + 1)) <= max_depth) continue;
    size_t held = 0;
    for (size_t i = 0; i < before;) {
      size_t r = i, m = 0; while (r < before && sp[r].first == sp[i].first) { m += sp[r].second > a; r++; }
      held += m;
      if (m >= 2 && held > max_depth) refuse(sp[i].first, held);
      i = r;
    }
  }
  return wide;
}

// index of the interval of an ascending grid that holds position p: the last start <= p (-1: p lies in front of the first start)
inline int64_t interval_of(const std::vector<uint32_t>& starts, int64_t p) {
  return (int64_t)(std::upper_bound(starts.begin(), starts.end(), (uint32_t)std::max<int64_t>(p, 0)) - starts.begin()) - 1;
}

// The slot bitmap of a focus window read as ranks: bit p - win_start + MKP_SLOTBM_MARGIN is set where position p owns a tally column
// ("slot"), wpfx is the running popcount per word.
struct SlotRank {
  const std::vector<uint32_t>& slotbm; const std::vector<uint32_t>& wpfx; int64_t win_start, win_end;
  static size_t words_for(int64_t win) { return ((size_t)win + 2 * MKP_SLOTBM_MARGIN + 31) / 32 + 2; }
  uint32_t rank(int64_t p) const {   // slots in front of p (p inside the bitmap)
    const size_t b = (size_t)(p - win_start + MKP_SLOTBM_MARGIN);
    return wpfx[b >> 5] + (uint32_t)__builtin_popcount(slotbm[b >> 5] & ((1u << (b & 31)) - 1u)); }
  uint32_t crank(int64_t p) const {  // p clamped to the bitmap's margins
    return rank(std::min(std::max(p, win_start - (int64_t)MKP_SLOTBM_MARGIN), win_end + (int64_t)MKP_SLOTBM_MARGIN)); }
  uint32_t halo_slots(int64_t a, int64_t b) const { return crank(b + MKP_HALO) - crank(a - MKP_HALO); }   // tally columns of a tile [a, b)
};

// slot bitmap of a focus window, its running popcount per word and — slot pipeline — the slot positions.  Depends on the focus bytes only.
inline void window_slots(const ShardHost& S, const uint8_t* fz, const std::vector<mkp_motif_combo>& combos, bool hemi, bool stream,
                         std::vector<uint32_t>& slotbm, std::vector<uint32_t>& wpfx, std::vector<uint32_t>& slot_pos, SlotLists& lists) {
  const int64_t win = (int64_t)S.win_end - (int64_t)S.win_start;
  const size_t nwords = SlotRank::words_for(win);
  slotbm.assign(nwords, 0);
  // pileup-hemi: only the positions with a positive-strand motif hit own a column (positions_to_motifs.get(pos), duplex.rs:289-296)
  uint8_t hemi_ok[64]; for (size_t k = 0; k < 64; k++) hemi_ok[k] = (k < combos.size() && combos[k].n_pos > 0) ? 1 : 0;
  // pieces are multiples of 32 positions and the margin is 64: no two pieces share a word
  host_parallel((size_t)win, (size_t)1 << 20, [&](size_t lo, size_t hi) {
    for (size_t p = lo; p < hi; p++) if (hemi ? ((fz[p] & 1u) && hemi_ok[fz[p] >> 2]) : (fz[p] & 3u)) {
      const size_t b = p + MKP_SLOTBM_MARGIN; slotbm[b >> 5] |= 1u << (b & 31); }
  });
  wpfx.assign(nwords + 1, 0);
  {   // running popcount over the bitmap words: block sums on all cores, a short serial pass over the blocks, then the blocks again
    const size_t blk = (size_t)1 << 16, nblk = (nwords + blk - 1) / blk; std::vector<uint32_t> bsum(nblk + 1, 0);
    host_parallel(nblk, 1, [&](size_t lo, size_t hi) { for (size_t b = lo; b < hi; b++) { uint32_t t = 0;
        for (size_t w = b * blk; w < std::min(nwords, (b + 1) * blk); w++) t += (uint32_t)__builtin_popcount(slotbm[w]);
        bsum[b + 1] = t; } });
    for (size_t b = 0; b < nblk; b++) bsum[b + 1] += bsum[b];
    host_parallel(nblk, 1, [&](size_t lo, size_t hi) { for (size_t b = lo; b < hi; b++) { uint32_t run = bsum[b];
        for (size_t w = b * blk; w < std::min(nwords, (b + 1) * blk); w++) { wpfx[w] = run; run += (uint32_t)__builtin_popcount(slotbm[w]); } } });
    wpfx[nwords] = bsum[nblk];
  }
  slot_pos.clear();
  if (stream) {
    slot_pos.resize(wpfx[nwords]);
    host_parallel(nwords, (size_t)1 << 15, [&](size_t lo, size_t hi) {
      for (size_t w = lo; w < hi; w++) { uint32_t at = wpfx[w];
        for (uint32_t bits = slotbm[w]; bits; bits &= bits - 1u)
          slot_pos[at++] = (uint32_t)((int64_t)(w * 32 + (size_t)__builtin_ctz(bits)) - MKP_SLOTBM_MARGIN + S.win_start); }
    });
  }
  // The slot-entry lists (SlotLists, mkp_pack.hpp), from the same focus bytes: a row of strand s is emitted only where the rule has bit s
  // (E1 of pileup_stream_body, mkp_slots.hip), so a read that feeds one tally strand is only ever asked about that strand's slots.  Blocks
  // of bitmap words count their strand slots on all cores, a short serial pass sums the blocks, then every block writes its entries.
  lists.clear();
  if (stream) {
    const uint32_t n_all = wpfx[nwords];
    const size_t blk = (size_t)1 << 15, nblk = (nwords + blk - 1) / blk;
    std::vector<uint32_t> bs[2]; bs[0].assign(nblk + 1, 0); bs[1].assign(nblk + 1, 0);
    auto rule_at = [&](size_t w, uint32_t bit) { return (uint32_t)fz[w * 32 + bit - MKP_SLOTBM_MARGIN] & 3u; };   // (a set bit lies inside the window)
    host_parallel(nblk, 1, [&](size_t lo, size_t hi) { for (size_t b = lo; b < hi; b++) { uint32_t t0 = 0, t1 = 0;
        for (size_t w = b * blk; w < std::min(nwords, (b + 1) * blk); w++)
          for (uint32_t bits = slotbm[w]; bits; bits &= bits - 1u) { const uint32_t r = rule_at(w, (uint32_t)__builtin_ctz(bits)); t0 += r & 1u; t1 += r >> 1; }
        bs[0][b + 1] = t0; bs[1][b + 1] = t1; } });
    for (size_t b = 0; b < nblk; b++) { bs[0][b + 1] += bs[0][b]; bs[1][b + 1] += bs[1][b]; }
    lists.n_all = n_all; lists.n_strand[0] = bs[0][nblk]; lists.n_strand[1] = bs[1][nblk];
    lists.ent.resize((size_t)n_all + lists.n_strand[0] + lists.n_strand[1]);
    lists.rank[0].resize((size_t)n_all + 1); lists.rank[1].resize((size_t)n_all + 1);
    lists.rank[0][n_all] = lists.n_strand[0]; lists.rank[1][n_all] = lists.n_strand[1];
    MkpSlotEnt* const e_all = lists.ent.data(); MkpSlotEnt* const e_str[2] = {e_all + lists.list_off(1), e_all + lists.list_off(2)};
    host_parallel(nblk, 1, [&](size_t lo, size_t hi) { for (size_t b = lo; b < hi; b++) { uint32_t at[2] = {bs[0][b], bs[1][b]};
        for (size_t w = b * blk; w < std::min(nwords, (b + 1) * blk); w++) { uint32_t g = wpfx[w];
          for (uint32_t bits = slotbm[w]; bits; bits &= bits - 1u, g++) {
            const uint32_t bit = (uint32_t)__builtin_ctz(bits), r = rule_at(w, bit);
            const MkpSlotEnt e = {slot_pos[g], g};
            e_all[g] = e; lists.rank[0][g] = at[0]; lists.rank[1][g] = at[1];
            if (r & 1u) e_str[0][at[0]++] = e;
            if (r & 2u) e_str[1][at[1]++] = e;
          } } } });
  }
}
inline bool stream_pipeline(bool has_focus, bool hemi) { return has_focus && !hemi; }   // focus runs take the slot pipeline (mkp_slots.hip)

// What the planner reads.  The shard's headers are written too (event slices, slot ranges, probability-sum flags), the caller tables are
// rebuilt for the layouts the shard uses, a missing hemi interval grid becomes the window, a valid window pre-plan is taken over.
struct PlanInput {
  ShardHost& S; LayoutTables& tables; const std::vector<LayoutHost>& layouts; const CallerCfg& caller;
  bool has_focus; const PodVec<uint8_t>& focus; const std::vector<mkp_motif_combo>& combos;
  const std::vector<uint32_t>& iv_starts;   // the reference's interval grid (duplicate-name rule, depth guard); empty: one interval
  bool hemi; int32_t hemi_off; std::vector<uint32_t>& hemi_iv;
  uint32_t tile_positions; size_t n_partition_tags; WindowPlan& wplan; PlanKnobs knobs;
};

// What the planner makes: the arrays that go to the device and the scalars the context keeps for the launches.
struct ShardPlan {
  MkpRunParams prm; uint32_t hemi_codes[4][MKP_KMAX + 2] = {};
  uint32_t n_class[7] = {}, n_slot_class[3] = {}, read_ids_dec_off = 0;
  bool wide = false, stream = false, preplanned = false;
  std::vector<std::vector<uint32_t>> dup_groups;   // records of one name (of any partition key) that meet inside an interval
  std::vector<uint8_t> dup_member;                 // per read: in one of dup_groups and inside the window
  std::vector<uint32_t> class_list, slot_ids;
  std::vector<MkpTile> tiles; std::vector<MkpSTile> stiles; std::vector<uint32_t> slotbm, wpfx, slot_pos;
  SlotLists lists;                                 // the slot-entry lists of the window (slot pipeline)
  std::vector<uint32_t> ent_off, ent_cnt;          // per read of the fused decoder: its run of slot entries (plan_read_entries)
  std::vector<MkpDupCons> dup_cons; std::vector<MkpDupSeg> dup_segs;
  std::vector<MkpWork> work;
  uint32_t slot_cap = 0, focus_words = 0, words_per_slot = 0, lds_bytes = 0, n_tiles = 0;
  uint64_t n_slots_total = 0, cov_bytes = 0, plane_bytes = 0;
  uint64_t fused_swept = 0, fused_looked_up = 0;   // the fused reads' terms of the decoder's algorithmic bytes
  uint64_t fused_entries = 0, fused_slots = 0;     // slot entries the fused reads decode, of the slots they span
};

// ---- stage 1.  Hazard: the reference's ReadCache is keyed by read NAME (read_cache.rs:28-35); two kept records with one name in one
// interval share a cache entry there: the later one is answered from the earlier one's calls.  Found here, planned behind the tile plan
// (plan_name_owners needs the focus positions), reproduced by mkp_dup_events (mkp_slots.hip).
inline void find_shared_names(const PlanInput& in, ShardPlan& pl) {
  const ShardHost& S = in.S; const size_t nn = S.name_hash.size();
  // every thread takes the names whose hash falls into its sixteenth and looks for a repeat in an open-addressing table of its own
  // (value = the first record carrying the name); repeats are rare, so they are only collected here and judged below
  std::mutex dmu; std::vector<std::pair<uint32_t, uint32_t>> dups;   // (first record with the name, a later one)
  host_parallel(16, 1, [&](size_t lo, size_t hi) { for (size_t part = lo; part < hi; part++) {
    size_t mine = 0; for (size_t i = 0; i < nn; i++) if ((S.name_hash[i] >> 60) == part) mine++;
    if (mine < 2) continue;
    size_t cap = 64; while (cap < 2 * mine) cap <<= 1;
    std::vector<uint64_t> tab(cap, 0); std::vector<uint32_t> who(cap, 0); std::vector<uint8_t> used(cap, 0);
    // (by name alone, whatever the records' partition keys: the reference builds ONE read cache per interval for all keys and asks it by
    //  name, pileup/mod.rs:745, read_cache.rs:238; the key only chooses the tally a record's features and codes go to, mod.rs:795-835.  A
    //  group may span keys: a consumer's rebuilt list is counted in the pass of the consumer's own key)
    for (size_t i = 0; i < nn; i++) {
      const uint64_t hh = S.name_hash[i]; if ((hh >> 60) != part) continue;
      size_t at = (size_t)((hh * 0x9e3779b97f4a7c15ull) >> 20) & (cap - 1);
      for (;;) {
        if (!used[at]) { used[at] = 1; tab[at] = hh; who[at] = (uint32_t)i; break; }
        if (tab[at] == hh) { std::lock_guard<std::mutex> g(dmu); dups.push_back({who[at], (uint32_t)i}); break; }
        at = (at + 1) & (cap - 1);
      }
    }
  } });
  // The reference keys its read cache by NAME, one cache per interval (read_cache.rs:28-35, pileup/mod.rs:718-760): two kept records
  // with one name meet only if they overlap a common interval — then the later one is answered from the earlier one's calls, which the
  // device path does not reproduce.  Mates / split alignments that lie in different intervals never share a cache and are simply two reads.
  // (No interval grid given: the shard is one interval.)
  // Every pair of records of one name is judged (three records A, B, C: the table above names (A, B) and (A, C); B and C can meet too).
  // A record that lies wholly outside the shard window — a halo record of the fetch — belongs to none of its intervals.
  std::map<uint32_t, std::vector<uint32_t>> groups;
  for (auto& d : dups) {
    if (d.first >= S.hdr.size() || d.second >= S.hdr.size()) continue;
    auto& g = groups[d.first];
    if (g.empty()) g.push_back(d.first);
    g.push_back(d.second);
  }
  auto iv_range = [&](const MkpReadHdr& h, int64_t* a, int64_t* b) -> bool {   // false: outside the window
    const int64_t s0 = h.ref_start, e0 = std::max<int64_t>(h.ref_end, (int64_t)h.ref_start + 1);
    if (e0 <= (int64_t)S.win_start || s0 >= (int64_t)S.win_end) return false;
    if (in.iv_starts.empty()) { *a = 0; *b = 0; return true; }
    *a = std::max<int64_t>(interval_of(in.iv_starts, std::max<int64_t>(s0, S.win_start)), 0);
    *b = std::max<int64_t>(interval_of(in.iv_starts, std::min<int64_t>(e0, S.win_end) - 1), 0);
    return true;
  };
  for (auto& kv : groups) {
    std::vector<uint32_t> g = kv.second; std::sort(g.begin(), g.end()); g.erase(std::unique(g.begin(), g.end()), g.end());
    std::vector<std::pair<int64_t, int64_t>> rg; rg.reserve(g.size());
    for (uint32_t r : g) { int64_t a, b; if (iv_range(S.hdr[r], &a, &b)) rg.push_back({a, b}); }
    bool meet = false;
    for (size_t x = 0; x < rg.size() && !meet; x++) for (size_t y = x + 1; y < rg.size(); y++)
      if (rg[x].first <= rg[y].second && rg[y].first <= rg[x].second) { meet = true; break; }
    if (!meet) continue;
    // pileup-hemi keys its DuplexReadCache by name as well (read_cache.rs:368-468); that form is not reproduced
    if (in.hemi) throw Error(MKP_E_UNSUPPORTED,
        "two primary records share a read name inside one interval (unmarked duplicates, or mates / split reads that overlap the same interval); pileup-hemi answers the later record from the earlier one's calls (its per-interval cache is keyed by name) and this is not reproduced on the device");
    pl.dup_groups.push_back(std::move(g));
  }
}

// pileup-hemi counters: a pattern block of (1 + codes)^2 counters per primary base that has calls, elements in DuplexModCodeRepr
// order (Canonical < Code(char) < ChEbi(id) = 0 < the code_repr encoding's numeric order)
inline void build_hemi_params(const PlanInput& in, ShardPlan& pl) {
  ShardHost& S = in.S; MkpRunParams& P = pl.prm; const SlotTable& st = in.tables.st;
  if (!in.has_focus) throw Error(MKP_E_INVALID, "pileup-hemi needs the focus positions of a palindromic motif");
  if (in.n_partition_tags) throw Error(MKP_E_INVALID, "pileup-hemi has no partition tags");
  P.hemi = 1; P.hemi_off = in.hemi_off;
  memset(P.hemi_el, 0xff, sizeof(P.hemi_el)); memset(pl.hemi_codes, 0, sizeof(pl.hemi_codes));
  uint32_t next = MKP_H_PAT;
  for (int b = 0; b < 4; b++) { P.hemi_pat_base[b] = 0xff; P.hemi_nel[b] = 0; }
  for (size_t k = 0; k < st.can_pbs.size(); k++) {
    const int pb = st.can_pbs[k];
    std::vector<int> mine; for (size_t i = 0; i < st.slots.size(); i++) if (st.slots[i].pb == pb) mine.push_back((int)i);
    std::sort(mine.begin(), mine.end(), [&](int x, int y) { return st.slots[(size_t)x].code_repr < st.slots[(size_t)y].code_repr; });
    const bool comb = P.numeric_mode == 1;   // DuplexModCall::into_combined: every modified element becomes the base's any-mod code
    const uint32_t nel = comb ? (mine.empty() ? 1u : 2u) : 1u + (uint32_t)mine.size();
    if (nel > MKP_KMAX + 1) throw Error(MKP_E_UNSUPPORTED, "more mod codes on one base than a pileup-hemi pattern block holds");
    P.hemi_pat_base[pb] = (uint8_t)next; P.hemi_nel[pb] = (uint8_t)nel; next += nel * nel;
    P.hemi_el[MKP_C_CAN + k] = 0;
    for (size_t r = 0; r < mine.size(); r++) {
      const MkpSlot& sl = st.slots[(size_t)mine[r]];
      P.hemi_el[sl.cid] = (uint8_t)(comb ? 1u : 1u + r);
      pl.hemi_codes[pb][comb ? 1u : 1u + r] = comb ? (uint32_t)"ACGT"[pb] : sl.code_repr;
    }
  }
  if (next > MKP_H_MAX_COUNTERS) throw Error(MKP_E_UNSUPPORTED, "too many pileup-hemi pattern counters for one LDS tile");
  P.hemi_counters = next;
  // a record whose tags fail leaves one NoCall per interval it crosses (mkp_hemi_failed_reads), written into its own event slice:
  // make every slice at least that long
  if (in.hemi_iv.empty()) in.hemi_iv.push_back((uint32_t)S.win_start);
  if (!std::is_sorted(in.hemi_iv.begin(), in.hemi_iv.end())) throw Error(MKP_E_INVALID, "interval starts must ascend");
  for (auto& h : S.hdr) {
    // (counted in intervals begun at or in front of a position: interval_of + 1, and the two + 1 cancel)
    const int64_t need = interval_of(in.hemi_iv, (int64_t)h.ref_end - 1) - interval_of(in.hemi_iv, h.ref_start) + 1;
    h.event_cap = (uint32_t)std::max<int64_t>(h.event_cap, need);
  }
}

// ---- stage 2.  Caller tables over the layouts this shard's reads use (not whatever the packer has interned before), the run
// parameters, the slot order and — pileup-hemi — the pattern counters.
inline void build_params(const PlanInput& in, ShardPlan& pl) {
  const ShardHost& S = in.S; const CallerCfg& cc = in.caller;
  { std::vector<uint8_t> used(in.layouts.size(), 0);
    for (auto& h : S.hdr) if (!(h.flags & MKP_RF_BAD) && h.n_tags && h.layout < used.size()) used[h.layout] = 1;
    in.tables.build(in.layouts, cc, &used); }
  const SlotTable& st = in.tables.st;
  MkpRunParams& P = pl.prm; memset(&P, 0, sizeof(P));
  P.win_start = S.win_start; P.win_end = S.win_end;
  P.n_counters = in.tables.n_counters; P.n_slots = (uint32_t)st.slots.size(); P.n_pb = (uint32_t)st.can_pbs.size();
  P.numeric_mode = cc.numeric_mode; P.combine_strands = cc.combine_strands; P.edge_filter = cc.edge; P.edge_start = cc.edge_start;
  P.edge_end = cc.edge_end; P.edge_inverted = cc.edge_inverted; P.force_allow = cc.force_allow; P.max_depth = cc.max_depth;
  P.has_focus = in.has_focus; P.n_combos = (uint32_t)in.combos.size();
#ifdef MKP_DEBUG
  P.debug_skip = in.knobs.debug_skip;
#endif
  for (int b = 0; b < 4; b++) { P.can_of_pb[b] = 0xff; P.pb_of_can[b] = 0; }
  for (size_t k = 0; k < st.can_pbs.size(); k++) { P.can_of_pb[st.can_pbs[k]] = (uint8_t)k; P.pb_of_can[k] = (uint8_t)st.can_pbs[k]; }
  std::vector<int> order(P.n_slots); for (uint32_t i = 0; i < P.n_slots; i++) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    const MkpSlot &x = st.slots[(size_t)a], &y = st.slots[(size_t)b]; return x.code_repr != y.code_repr ? x.code_repr < y.code_repr : x.pb < y.pb; });
  for (uint32_t i = 0; i < P.n_slots; i++) { P.slot_order[i] = (uint8_t)order[i]; P.slots[i] = st.slots[i]; }
  if (P.combine_strands && !P.has_focus) throw Error(MKP_E_INVALID, "combine_strands needs motif focus positions");
  if (in.hemi) build_hemi_params(in, pl);
}

// ---- stage 4.  SPARSE reads with two tags: combine_checked's test (mod_bam.rs:629-656) that a call's probabilities over both tags do
// not add up to more than 1.01 — every term is (2q + 1) / 512, so the f32 sum is exact and `> 1.01f` is "the numerators reach 518" — is
// made here over the ML bytes, on all cores, and handed to the slot decoder as a header flag
inline void flag_sum_errors(const PlanInput& in, const ShardPlan& pl) {
  ShardHost& S = in.S; const uint32_t* two_tag = pl.class_list.data() + pl.n_class[0];
  host_parallel(pl.n_class[1], 2048, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      MkpReadHdr& h = S.hdr[two_tag[k]];
      if (S.dev_packed) { if (S.dev_sum2[two_tag[k]]) h.flags |= MKP_RF_SUMERR; else h.flags &= ~MKP_RF_SUMERR; continue; }
      const MkpLayout& L = in.tables.dev[h.layout];
      const MkpTagRef &t0 = S.tagref[h.tag_off], &t1 = S.tagref[h.tag_off + 1];
      const uint32_t nc0 = L.tags[0].n_codes, nc1 = L.tags[1].n_codes;
      bool bad = false;
      for (uint32_t j = 0; j < t0.n && !bad; j++) {
        uint32_t num = 0;
        for (uint32_t i = 0; i < nc0; i++) num += 2u * S.ml[t0.ml_off + j * nc0 + i] + 1u;
        for (uint32_t i = 0; i < nc1; i++) num += 2u * S.ml[t1.ml_off + j * nc1 + i] + 1u;
        bad = num >= 518u;
      }
      if (bad) h.flags |= MKP_RF_SUMERR; else h.flags &= ~MKP_RF_SUMERR;
    }
  });
}

// ---- stage 5.  A duplex read decoded one group per wave needs room for both groups' lists behind the merged one; then the event slices
// are laid out again (capacities may have grown here and in build_hemi_params).
inline void layout_event_slices(const PlanInput& in, ShardPlan& pl) {
  ShardHost& S = in.S;
  size_t at = 0; for (int k = 0; k < 5; k++) at += pl.n_class[k];
  for (; at < pl.class_list.size(); at += 2) {
    MkpReadHdr& h = S.hdr[pl.class_list[at]];
    const uint64_t need = 2ull * ((uint64_t)S.tagref[h.tag_off].n + S.tagref[h.tag_off + in.tables.dev[h.layout].pad].n);
    if (need > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 call events in one read");
    h.event_cap = std::max(h.event_cap, (uint32_t)need);
  }
  uint64_t off = 0;
  for (auto& h : S.hdr) {
    if (off > 0xfffffff0ull - h.event_cap) throw Error(MKP_E_UNSUPPORTED, "shard exceeds 4 Gi call events; use smaller shards");
    h.event_off = (uint32_t)off; off += h.event_cap;
  }
  S.n_events_cap = off;
  pl.prm.readout_b_off = (uint32_t)S.hdr.size();
}

// ---- stage 6.  The sweeps below need the records in coordinate order; the depth guard decides the tally width.
inline void check_sorted_and_depth(const PlanInput& in, ShardPlan& pl) {
  const ShardHost& S = in.S;
  for (size_t i = 1; i < S.hdr.size(); i++)
    if (S.hdr[i].ref_start < S.hdr[i - 1].ref_start) throw Error(MKP_E_INVALID, "records must be coordinate sorted");
  pl.wide = depth_guard(S, in.caller.max_depth, in.iv_starts, in.hemi);
}

// ---- stage 7: the tile plan.  The accumulate kernel runs two 1024-thread workgroups per CU, each holding one tile in LDS: 76 KiB per
// workgroup including ~3.5 KiB of static LDS leaves slack for the allocation granule (at 80 KiB each one GPU box ran them one
// per CU and the kernel took 1.9x as long).  A tile = a run of reference positions; its tally columns ("slots") are all of
// its positions, or — when the run has focus positions — only those, so a --cpg tile spans ~50x more reference.  A wide shard holds
// two u32 planes per counter (one per strand): twice the tally words per slot, so about half the slots per tile.
constexpr uint32_t kTileBudgetWords = (76u * 1024u - 3584u) / 4u;
inline uint32_t max_slots_for(uint32_t words_per_slot, uint32_t focus_words) {
  uint32_t best = 0;
  for (uint32_t s = 64; s <= 4160; s += 64) if (MKP_PILEUP_LDS_WORDS(words_per_slot, s, focus_words) <= kTileBudgetWords) best = s;
  return best;
}

// no focus: every position of the window owns a tally column
inline void plan_dense_tiles(const PlanInput& in, ShardPlan& pl) {
  const ShardHost& S = in.S;
  const uint32_t Smax = max_slots_for(pl.words_per_slot, 0);
  if (Smax < 128) throw Error(MKP_E_UNSUPPORTED, "too many counters for one LDS tile");
  uint32_t T = Smax - 2 * MKP_HALO;
  if (in.tile_positions) T = std::min(T, std::max<uint32_t>(32u, in.tile_positions));
  pl.slot_cap = (T + 2 * MKP_HALO + 63u) & ~63u;
  for (int64_t r0 = S.win_start; r0 < S.win_end; r0 += T) pl.tiles.push_back({(int32_t)r0, (int32_t)std::min<int64_t>(r0 + T, S.win_end), 0, 0});
}

// slot pipeline (mkp_slots.hip): global slot numbering, per-read slot ranges and feature-stream offsets, tiles of slots
inline void plan_slot_tiles(const PlanInput& in, ShardPlan& pl) {
  ShardHost& S = in.S; const SlotRank R{pl.slotbm, pl.wpfx, S.win_start, S.win_end};
  const uint32_t total = pl.wpfx[pl.slotbm.size()];
  host_parallel(S.hdr.size(), 8192, [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) { MkpReadHdr& h = S.hdr[i];
      const uint32_t a = R.crank(h.ref_start), b = std::max(a, R.crank(h.ref_end)); h.gs0 = a; h.n_sl = b - a; } });
  uint64_t off = 0;
  for (auto& h : S.hdr) {   // (the stream offsets are a running sum: serial, but nothing else is left in the loop)
    h.cov_off = (uint32_t)off;
    off += ((uint64_t)h.n_sl + 3u) & ~3ull;
    if (off > 0xffffff00ull) throw Error(MKP_E_UNSUPPORTED, "shard exceeds 4 GiB of per-read focus positions; use smaller shards");
  }
  pl.cov_bytes = off;
  // tile = a run of slots: rows for [g0, g1), tally columns for the slots within MKP_HALO positions of them (strand combining)
  // LDS of mkp_pileup_stream: tallies + per slot its position and an emission word, + the row map (one thread per slot decides the rows)
  const uint32_t Smax = std::min<uint32_t>(MKP_PILEUP_THREADS, ((kTileBudgetWords - MKP_STREAM_ROWMAP_WORDS) / (pl.words_per_slot + 2u)) & ~63u);
  if (Smax < 128) throw Error(MKP_E_UNSUPPORTED, "too many counters for one LDS tile");
  // as many slots per tile as LDS and the one-thread-per-slot emission allow, down to ~1024 tiles for small windows: a read is visited once
  // per tile it crosses and the visits are most of the kernel (C3, round 6: 448 / 640 / 704 / 896 / 992 slots: 0.153 / 0.139 / 0.128 /
  // 0.125 / 0.116 ms)
  uint32_t Te = std::min<uint32_t>(Smax - 2 * MKP_HALO, std::max<uint32_t>(256u, (total / 1024u + 63u) & ~63u));
  // tests: many small tiles
  if (in.tile_positions) Te = std::max<uint32_t>(32u, std::min<uint32_t>(Smax - 2 * MKP_HALO, in.tile_positions / 4u));
  // experiments
  if (in.knobs.has_stream_tile) Te = std::max<uint32_t>(32u, std::min<uint32_t>(Smax - 2 * MKP_HALO, in.knobs.stream_tile));
  uint32_t most = 0;
  for (uint32_t g0 = 0; g0 < total; g0 += Te) {
    MkpSTile t; t.g0 = g0; t.g1 = std::min(total, g0 + Te);
    t.r0 = (int32_t)pl.slot_pos[t.g0]; t.r1 = (int32_t)pl.slot_pos[t.g1 - 1u] + 1;
    t.gh0 = R.crank((int64_t)t.r0 - MKP_HALO); t.gh1 = R.crank((int64_t)t.r1 + MKP_HALO); t.first = t.last = 0;
    pl.stiles.push_back(t); most = std::max(most, t.gh1 - t.gh0);
  }
  if (most > Smax) throw Error(MKP_E_UNSUPPORTED, "internal: slot tile does not fit the LDS budget");
  pl.slot_cap = std::max<uint32_t>(64u, (most + 63u) & ~63u); pl.focus_words = 0;
}

// pileup-hemi keeps the tile walk over reference positions, with the focus positions as tally columns
inline void plan_focus_tiles(const PlanInput& in, ShardPlan& pl) {
  const ShardHost& S = in.S; const SlotRank R{pl.slotbm, pl.wpfx, S.win_start, S.win_end};
  const int64_t win = (int64_t)S.win_end - (int64_t)S.win_start;
  // span: enough tiles to balance 512 persistent workgroups, bounded by the bitmap the tile keeps in LDS
  const uint32_t span_max = 32768 - 128;
  // A read is visited once per tile it crosses: longer tiles mean fewer visits (10 kb reads: 1.64 per read at 16 kb, 1.41 at 24 kb),
  // fewer tiles mean a coarser balance over the 512 resident workgroups.  Measured on C3: 2 600 tiles of 24 kb beat 4 100 of 16 kb by 9 %
  // and 7 900 of 8 kb by 31 %.  Small windows keep >= 16 kb tiles (a handful of workgroups of little work each).
  uint32_t span = (uint32_t)std::min<int64_t>(span_max, std::max<int64_t>(16384, ((win / 2600) + 63) & ~63ll));
  // explicit tile span (tests: many small tiles; experiments: larger ones)
  if (in.tile_positions) span = std::max<uint32_t>(64u, std::min(span_max & ~63u, in.tile_positions & ~63u));
  pl.focus_words = (span + 2 * MKP_HALO + 31 + 31) / 32 + 2;
  // row emission of a focus tile: one thread per slot
  const uint32_t Smax = std::min<uint32_t>(max_slots_for(pl.words_per_slot, pl.focus_words), MKP_PILEUP_THREADS);
  if (Smax < 128) throw Error(MKP_E_UNSUPPORTED, "too many counters for one LDS tile");
  uint32_t most = 0;
  for (int64_t r0 = S.win_start; r0 < S.win_end;) {
    int64_t r1 = std::min<int64_t>(r0 + span, S.win_end);
    while (R.halo_slots(r0, r1) > Smax && r1 - r0 > 32) r1 = r0 + std::max<int64_t>(32, (r1 - r0) / 2);   // dense focus: shorter tile
    if (R.halo_slots(r0, r1) > Smax) throw Error(MKP_E_UNSUPPORTED, "internal: focus tile does not fit the LDS budget");
    // (a tile without focus positions emits nothing)
    if (R.rank(r1) > R.rank(r0)) { pl.tiles.push_back({(int32_t)r0, (int32_t)r1, 0, 0}); most = std::max(most, R.halo_slots(r0, r1)); }
    r0 = r1;
  }
  pl.slot_cap = std::max<uint32_t>(64u, (most + 63u) & ~63u);
}

inline void plan_tiles(const PlanInput& in, ShardPlan& pl) {
  const ShardHost& S = in.S; MkpRunParams& P = pl.prm;
  pl.words_per_slot = (in.hemi ? P.hemi_counters : P.n_counters + P.n_slots) * (pl.wide ? 2u : 1u);
  pl.stream = stream_pipeline(in.has_focus, in.hemi);
  P.slot_stream = pl.stream ? 1u : 0u;
  if (!in.has_focus) plan_dense_tiles(in, pl);
  else {
    // slot bitmap + running popcount + slot positions: made ahead of the reads when the driver asked for it (mkp_internal_shard_preplan)
    pl.preplanned = in.wplan.valid && pl.stream && !in.hemi
        && in.wplan.slotbm.size() == SlotRank::words_for((int64_t)S.win_end - (int64_t)S.win_start);
    if (pl.preplanned) { pl.slotbm.swap(in.wplan.slotbm); pl.wpfx.swap(in.wplan.wpfx); pl.slot_pos.swap(in.wplan.slot_pos);
      pl.lists.swap(in.wplan.lists); in.wplan.valid = false; }
    else window_slots(S, in.focus.data(), in.combos, in.hemi, pl.stream, pl.slotbm, pl.wpfx, pl.slot_pos, pl.lists);
    if (pl.stream) plan_slot_tiles(in, pl); else plan_focus_tiles(in, pl);
    for (size_t w = 0; w < pl.slotbm.size(); w++) pl.n_slots_total += (uint64_t)__builtin_popcount(pl.slotbm[w]);
  }
  P.slot_cap = pl.slot_cap; P.focus_words = pl.focus_words;
  pl.lds_bytes = pl.stream ? ((pl.words_per_slot + 2u) * pl.slot_cap + MKP_STREAM_ROWMAP_WORDS) * 4u
                           : MKP_PILEUP_LDS_WORDS(pl.words_per_slot, pl.slot_cap, pl.focus_words) * 4u;
}

// ---- stage 8: tile -> [first, last) candidate reads.  Reads are coordinate sorted, so in either coordinate (reference positions; slots:
// a read's first slots ascend too) the prefix-max of the reads' ends bounds the first candidate.  span(h) = {begin, end, may the read
// count} of a read, range(tile) = {lo, hi} of the tile's halo range; a tile no counting read reaches is dropped.
struct ReadSpan { int64_t beg, end; bool counts; };
template <class Tile, class Span, class Range> void sweep_candidates(const ShardHost& S, std::vector<Tile>& tiles, Span span, Range range) {
  const size_t n = S.hdr.size();
  std::vector<int64_t> pmax(n); int64_t m = INT64_MIN;
  for (size_t i = 0; i < n; i++) { m = std::max(m, span(S.hdr[i]).end); pmax[i] = m; }
  size_t first = 0, last = 0; std::vector<Tile> kept;
  for (auto& tl : tiles) {
    const std::pair<int64_t, int64_t> r = range(tl);
    while (first < n && pmax[first] <= r.first) first++;
    if (last < first) last = first;
    while (last < n && span(S.hdr[last]).beg < r.second) last++;
    bool any = false;
    for (size_t i = first; i < last && !any; i++) { const ReadSpan s = span(S.hdr[i]); any = s.end > r.first && s.counts; }
    if (any) { tl.first = (uint32_t)first; tl.last = (uint32_t)last; kept.push_back(tl); }
  }
  tiles.swap(kept);
}
inline void candidate_reads(const PlanInput& in, ShardPlan& pl) {
  sweep_candidates(in.S, pl.tiles, [](const MkpReadHdr& h) { return ReadSpan{h.ref_start, h.ref_end, true}; },
      [](const MkpTile& t) { return std::pair<int64_t, int64_t>{(int64_t)t.r0 - MKP_HALO, (int64_t)t.r1 + MKP_HALO}; });
  if (pl.stream) sweep_candidates(in.S, pl.stiles,
      [](const MkpReadHdr& h) { return ReadSpan{h.gs0, (int64_t)h.gs0 + h.n_sl, h.n_sl > 0}; },
      [](const MkpSTile& t) { return std::pair<int64_t, int64_t>{t.gh0, t.gh1}; });
  pl.n_tiles = pl.stream ? (uint32_t)pl.stiles.size() : (uint32_t)pl.tiles.size();
}

// ---- stage 9: records sharing a name inside an interval (dup_groups): who answers for the name in which interval.
// The reference asks its per-interval cache about a record the first time the record shows up in a focus column of the interval as
// something other than a reference skip (add_mod_codes_for_record is called before the deletion check, pileup/mod.rs:783-835); columns
// ascend, records inside a column come in file order.  The first record asked OWNS the name in that interval: its tags are parsed, its
// calls (by reference position and read base), its codes and its failure answer for every record of the name (read_cache.rs:232-355).
// `dev_cigar(read)`: the CIGAR of a read of a device-packed shard (the host holds none).
using CigarFetch = std::function<std::vector<uint32_t>(uint32_t)>;
struct DupMember { uint32_t r; int64_t beg, end; std::vector<std::pair<int64_t, int64_t>> skips; };
// first column of [lo, hi) in which member m is asked about: a focus position that is not inside one of its reference skips
inline int64_t first_asked_column(const DupMember& m, int64_t lo, int64_t hi, bool has_focus, const std::vector<uint32_t>& slot_pos) {
  lo = std::max(lo, m.beg); hi = std::min(hi, m.end);
  auto in_skip = [&](int64_t p, int64_t* e) {
    for (auto& sk : m.skips) if (p >= sk.first && p < sk.second) { *e = sk.second; return true; }
    return false; };
  if (!has_focus) { int64_t p = lo, e; while (p < hi && in_skip(p, &e)) p = e; return p < hi ? p : -1; }
  for (size_t k = (size_t)(std::lower_bound(slot_pos.begin(), slot_pos.end(), (uint32_t)std::max<int64_t>(lo, 0)) - slot_pos.begin());
       k < slot_pos.size() && (int64_t)slot_pos[k] < hi; k++) {
    int64_t e; if (!in_skip((int64_t)slot_pos[k], &e)) return (int64_t)slot_pos[k]; }
  return -1;
}
inline void plan_name_owners(const PlanInput& in, ShardPlan& pl, const CigarFetch& dev_cigar) {
  ShardHost& S = in.S;
  pl.dup_member.assign(S.hdr.size(), 0);
  if (pl.dup_groups.empty()) return;
  auto cigar_of = [&](uint32_t r) {
    if (S.dev_packed) return dev_cigar(r);
    const MkpReadHdr& h = S.hdr[r]; std::vector<uint32_t> cg(h.n_cigar);
    for (uint32_t k = 0; k < h.n_cigar; k++) cg[k] = S.cigar[h.cigar_off + k];
    return cg;
  };
  const int64_t W0 = S.win_start, W1 = S.win_end; const std::vector<uint32_t>& iv = in.iv_starts;
  auto iv_bounds = [&](int64_t k, int64_t* a, int64_t* b) {   // interval k of the shard's grid, clipped to the window
    if (iv.empty()) { *a = W0; *b = W1; return; }
    *a = std::max<int64_t>(W0, k == 0 ? W0 : (int64_t)iv[(size_t)k]);
    *b = (size_t)k + 1 < iv.size() ? std::min<int64_t>(W1, (int64_t)iv[(size_t)k + 1]) : W1;
  };
  auto iv_index = [&](int64_t p) -> int64_t { return iv.empty() ? 0 : std::max<int64_t>(interval_of(iv, p), 0); };
  uint64_t ev_off = S.n_events_cap;
  for (auto& g : pl.dup_groups) {
    std::vector<DupMember> ms;
    for (uint32_t r : g) {
      const MkpReadHdr& h = S.hdr[r]; DupMember m; m.r = r; m.beg = h.ref_start; m.end = std::max<int64_t>(h.ref_end, (int64_t)h.ref_start + 1);
      if (m.end <= W0 || m.beg >= W1) continue;   // a halo record of the fetch: in none of the shard's intervals
      int64_t p = h.ref_start;
      for (uint32_t w : cigar_of(r)) {
        const uint32_t op = w & 15u, len = w >> 4;
        if (op == 3u) m.skips.push_back({p, p + len});
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) p += len;
      }
      ms.push_back(std::move(m)); pl.dup_member[r] = 1;
    }
    int64_t k_lo = INT64_MAX, k_hi = -1;
    for (auto& m : ms) { k_lo = std::min(k_lo, iv_index(std::max(m.beg, W0))); k_hi = std::max(k_hi, iv_index(std::min(m.end, W1) - 1)); }
    std::vector<std::vector<MkpDupSeg>> segs_of(ms.size());
    for (int64_t k = k_lo; k <= k_hi; k++) {
      int64_t a, b; iv_bounds(k, &a, &b);
      int64_t best_p = -1; size_t best = 0; std::vector<uint8_t> present(ms.size(), 0);
      for (size_t x = 0; x < ms.size(); x++) {
        const int64_t fc = first_asked_column(ms[x], a, b, in.has_focus, pl.slot_pos); if (fc < 0) continue;
        present[x] = 1;
        if (best_p < 0 || fc < best_p) { best_p = fc; best = x; }   // (members are in file order: the first of equal columns stays)
      }
      if (best_p < 0) continue;
      for (size_t x = 0; x < ms.size(); x++) if (present[x]) {
        auto& sv = segs_of[x]; const uint32_t owner = ms[best].r;
        if (!sv.empty() && sv.back().owner == owner && sv.back().p_hi == (int32_t)a) sv.back().p_hi = (int32_t)b;
        else sv.push_back({(int32_t)a, (int32_t)b, S.hdr[owner].event_off, owner});
      }
    }
    for (size_t x = 0; x < ms.size(); x++) {
      bool foreign = false; for (auto& sg : segs_of[x]) if (sg.owner != ms[x].r) foreign = true;
      if (!foreign) continue;   // asked about first wherever it shows up: an ordinary record (whose events others may read)
      MkpDupCons dc; memset(&dc, 0, sizeof(dc));
      dc.rid = ms[x].r; dc.seg_off = (uint32_t)pl.dup_segs.size(); dc.n_seg = (uint32_t)segs_of[x].size(); dc.own_off = S.hdr[ms[x].r].event_off;
      uint64_t cap = 0; for (auto& sg : segs_of[x]) { cap += S.hdr[sg.owner].event_cap; pl.dup_segs.push_back(sg); }
      if (ev_off + cap > 0xfffffff0ull) throw Error(MKP_E_UNSUPPORTED, "shard exceeds 4 Gi call events; use smaller shards");
      dc.eff_off = (uint32_t)ev_off; dc.eff_cap = (uint32_t)cap; ev_off += cap;
      pl.dup_cons.push_back(dc);
    }
  }
  S.n_events_cap = ev_off;
}

// ---- stage 10: reads by kernel on the slot pipeline.  The fused slot decoder takes the SPARSE classes when no edge filter is set (it
// never locates calls off the focus positions, which the edge filter's "any call left" test would need); every other read is decoded into
// events by its class kernel and then covered.
// The slot entries a fused read decodes.  It writes coverage features on tally strand `aln` and call features on `aln ^ sg0` (sg0: the mod
// strand of its tags, MkpFusedDesc.misc bit 2), and a slot whose rule lacks bit s yields no row that reads a strand-s tally or a strand-s
// observed-code plane.  A read that needs one tally strand s therefore decodes its run of strand s's list — where that list is strictly
// shorter than `all` in this shard — and every other read (both strands needed; MKP_STRAND_SLOTS=0) its run of `all`.
inline void plan_read_entries(const PlanInput& in, ShardPlan& pl, uint32_t nf) {
  const ShardHost& S = in.S; const SlotLists& Ls = pl.lists;
  pl.ent_off.assign(S.hdr.size(), 0); pl.ent_cnt.assign(S.hdr.size(), 0);
  std::vector<uint8_t> sg0(in.tables.dev.size());
  for (size_t i = 0; i < sg0.size(); i++) sg0[i] = (uint8_t)((fused_desc(in.tables.dev[i]).misc >> 2) & 1u);
  host_parallel(nf, 8192, [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; k++) {
      const uint32_t r = pl.slot_ids[k]; const MkpReadHdr& h = S.hdr[r];
      const uint32_t aln = (h.flags & MKP_RF_REVERSE) ? 1u : 0u;
      const bool may_call = !(h.flags & MKP_RF_BAD) && h.n_tags != 0 && h.layout < sg0.size();
      const bool both = may_call && sg0[h.layout] != 0;   // calls go to the other tally strand
      if (!in.knobs.strand_slots_off && !both && Ls.n_strand[aln] < Ls.n_all) {
        const uint32_t a = Ls.rank[aln][h.gs0], b = Ls.rank[aln][h.gs0 + h.n_sl];
        pl.ent_off[r] = Ls.list_off(1 + (int)aln) + a; pl.ent_cnt[r] = b - a;
      } else { pl.ent_off[r] = h.gs0; pl.ent_cnt[r] = h.n_sl; }
    } });
}

inline void split_fused_and_cover(const PlanInput& in, ShardPlan& pl) {
  const ShardHost& S = in.S; const size_t n = S.hdr.size();
  if (!pl.stream) return;
  const bool fused = !pl.prm.edge_filter && !in.knobs.fused_off;
  std::vector<uint8_t> is_fused(n, 0);
  if (fused) {
    uint32_t dup_forced[2] = {0, 0};
    std::vector<uint32_t>& cl = pl.class_list;
    // (records sharing a name inside an interval keep their event decoder: their events are what the others are answered from; they move
    //  behind the fused reads of the class list, where the decode launch starts)
    if (!pl.dup_groups.empty()) {
      std::vector<uint32_t> keep, f0, f1; const uint32_t n0 = pl.n_class[0], n01 = pl.n_class[0] + pl.n_class[1]; uint32_t k0 = 0;
      for (uint32_t k = 0; k < n01; k++) {
        const uint32_t r = cl[k];
        if (pl.dup_member[r]) (k < n0 ? f0 : f1).push_back(r); else { keep.push_back(r); if (k < n0) k0++; }
      }
      std::vector<uint32_t> nl(keep); nl.insert(nl.end(), f0.begin(), f0.end()); nl.insert(nl.end(), f1.begin(), f1.end());
      nl.insert(nl.end(), cl.begin() + n01, cl.end());
      cl.swap(nl); pl.n_class[0] = k0; pl.n_class[1] = (uint32_t)keep.size() - k0;
      dup_forced[0] = (uint32_t)f0.size(); dup_forced[1] = (uint32_t)f1.size();
    }
    const uint32_t nf = pl.n_class[0] + pl.n_class[1];
    for (uint32_t k = 0; k < nf; k++) is_fused[cl[k]] = 1;
    // one list for both SPARSE classes, longest first (the longest reads start first: they do not make the launch's tail)
    pl.slot_ids.resize(nf);
    auto longer = [&](uint32_t x, uint32_t y) { return S.hdr[x].l_seq > S.hdr[y].l_seq; };
    std::merge(cl.begin(), cl.begin() + pl.n_class[0], cl.begin() + pl.n_class[0], cl.begin() + nf, pl.slot_ids.begin(), longer);
    // a wave's time goes with the slots it decodes: the launch order is by entry count (reads of one count keep their order by length)
    plan_read_entries(in, pl, nf);
    stable_sort_desc(pl.slot_ids, [&](uint32_t x) { return pl.ent_cnt[x]; });
    pl.n_slot_class[0] = nf;
    pl.read_ids_dec_off = nf; pl.n_class[0] = dup_forced[0]; pl.n_class[1] = dup_forced[1];
  }
  std::vector<uint32_t> rest; rest.reserve(n);
  for (size_t i = 0; i < n; i++) if (!is_fused[i]) rest.push_back((uint32_t)i);
  stable_sort_desc(rest, [&](uint32_t x) { return S.hdr[x].n_sl; });
  pl.n_slot_class[2] = (uint32_t)rest.size();
  pl.slot_ids.insert(pl.slot_ids.end(), rest.begin(), rest.end());
}

// ---- stage 11: the fused decoder's work records, in launch order, with their places in the call plane and the base plane
// (MKP_PLANE_WORDS(l_seq) 8-byte entries per fused read in either); what the SEQ sweep and rank marking would read of these reads and what
// the plane lookups read instead (the decoder's algorithmic bytes)

// What one pass reads of the planes for one fused read that decodes n_ent slots.  The gather is one 8-byte entry per slot, of the call
// plane for a read with calls and of the base plane for every other: at most one per entry of the read.  A read with calls also asks the
// base plane for 4 bytes under every match slot without a listed call.  The host does not know which slots those are; it knows that at
// most n_calls of the n_ent slots carry a listed call, so n_ent - n_calls (0 when there are more calls than slots) is the fewest base
// requests a read of matches makes.  This is a BOUND in the sense of the other algorithmic bytes — what the pass cannot do without, not
// what the hardware moves: a slot under a deletion or a ref-skip asks for nothing, and calls away from focus positions leave more slots
// unlisted than it counts.
inline uint64_t plane_lookup_bytes(uint32_t l_seq, uint32_t n_ent, bool with_calls, uint32_t n_calls) {
  const uint64_t gather = 8ull * std::min<uint64_t>(MKP_PLANE_WORDS(l_seq), n_ent);
  return gather + (with_calls && n_ent > n_calls ? 4ull * (n_ent - n_calls) : 0ull);
}
inline void build_work_records(const PlanInput& in, ShardPlan& pl) {
  const ShardHost& S = in.S;
  if (!pl.stream) return;
  const uint32_t nf = pl.n_slot_class[0];
  std::atomic<uint64_t> fused_swept{0}, fused_looked_up{0}, fused_entries{0}, fused_slots{0};
  pl.work.resize(nf);
  host_parallel(nf, 8192, [&](size_t lo, size_t hi) {
    uint64_t swept = 0, looked_up = 0, entries = 0, slots = 0;
    for (size_t k = lo; k < hi; k++) {
      const MkpReadHdr& h = S.hdr[pl.slot_ids[k]]; MkpWork& w = pl.work[k]; memset(&w, 0, sizeof(w));
      w.ref_start = h.ref_start; w.l_seq = h.l_seq; w.n_cigar = h.n_cigar;
      w.cigar_off = (h.flags & MKP_RF_CIGW) ? h.cigar_off : h.cigar16_off;   // the decoder's array of this read (MkpWork, mkp_device.h)
      w.seq_off = h.seq_off; w.flags = h.flags; w.gs0 = h.gs0; w.n_sl = h.n_sl;
      w.cov_off = h.cov_off; w.n_tags = h.n_tags; w.layout = h.layout; w.rid = pl.slot_ids[k];
      w.ent_off = pl.ent_off[w.rid]; w.n_ent = pl.ent_cnt[w.rid];
      if (!(h.flags & MKP_RF_BAD) && h.n_tags) {
        const MkpTagRef& t0 = S.tagref[h.tag_off]; w.rank_off = t0.rank_off; w.n_calls = t0.n; w.ml_off0 = t0.ml_off;
        if (h.n_tags > 1) w.ml_off1 = S.tagref[h.tag_off + 1].ml_off;
      }
      uint64_t n_rk = 0; if (!(h.flags & MKP_RF_BAD)) for (uint32_t t = 0; t < h.n_tags; t++) n_rk += S.tagref[h.tag_off + t].n;
      swept += (h.l_seq + 1) / 2 + 2ull * n_rk + ((h.flags & MKP_RF_CIGW) ? 0ull : 2ull * h.n_cigar);   // (16-bit CIGAR: 2 of the 4 bytes per op)
      // (a read with calls as the decoder sees it, but for a run-over delta list, which only mkp_call_plane finds)
      looked_up += plane_lookup_bytes(h.l_seq, w.n_ent, w.n_calls != 0 && !(h.flags & MKP_RF_SUMERR), w.n_calls);
      entries += w.n_ent; slots += h.n_sl;
    }
    fused_swept += swept; fused_looked_up += looked_up; fused_entries += entries; fused_slots += slots;
  });
  pl.fused_swept = fused_swept.load(); pl.fused_looked_up = fused_looked_up.load();
  pl.fused_entries = fused_entries.load(); pl.fused_slots = fused_slots.load();
  uint64_t pw = 0;
  for (uint32_t k = 0; k < nf; k++) {
    if (pw > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "shard exceeds 2^32 call-plane words; use smaller shards");
    pl.work[k].pad = (uint32_t)pw; pw += MKP_PLANE_WORDS(pl.work[k].l_seq);
  }
  pl.plane_bytes = pw * (sizeof(MkpCallEnt) + sizeof(MkpBaseEnt));   // the call plane, the base plane behind it
}

}  // namespace mkp
