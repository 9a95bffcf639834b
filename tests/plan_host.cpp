// Host program of tests/test_plan_host.py: the shard planner's stages (modkit_amd/csrc/mkp_plan.hpp) on read headers written by hand — no
// BAM records, no device.  Reads a scenario as whitespace-separated numbers:
//   win_start win_end tile_positions
//   n_focus focus positions..          (0: no focus, every position owns a column)
//   n_intervals interval starts..
//   n_reads, then per read: ref_start ref_end event_cap name_hash(hex) n_cigar (len op)..
// runs the stages in the planner's order and prints what they made as text; a refusal is printed as `error <status> <message>`.
#include <cinttypes>
#include <cstdio>

#include "mkp_plan.hpp"

using namespace mkp;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r"); if (!f) return 2;
  auto num = [&]() { long long v = 0; if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short scenario\n"); exit(2); } return v; };
  ShardHost S; LayoutTables T; std::vector<LayoutHost> layouts; CallerCfg cc; WindowPlan wp;
  S.win_start = (int32_t)num(); S.win_end = (int32_t)num(); const uint32_t tile_positions = (uint32_t)num();
  const size_t n_focus = (size_t)num();
  PodVec<uint8_t> focus; std::vector<mkp_motif_combo> combos;
  if (n_focus) {
    focus.assign((size_t)(S.win_end - S.win_start), 0);
    for (size_t k = 0; k < n_focus; k++) focus[(size_t)(num() - S.win_start)] = 1;   // a positive-strand hit of motif combo 0
    mkp_motif_combo z; memset(&z, 0, sizeof(z)); combos.push_back(z);
  }
  std::vector<uint32_t> iv_starts((size_t)num()), hemi_iv; for (auto& x : iv_starts) x = (uint32_t)num();
  const size_t n = (size_t)num();
  for (size_t i = 0; i < n; i++) {
    MkpReadHdr h; memset(&h, 0, sizeof(h));
    h.ref_start = (int32_t)num(); h.ref_end = (int32_t)num(); h.event_cap = (uint32_t)num(); h.l_seq = (uint32_t)(h.ref_end - h.ref_start);
    unsigned long long name = 0; if (fscanf(f, "%llx", &name) != 1) return 2;
    h.n_cigar = (uint32_t)num(); h.cigar_off = (uint32_t)S.cigar.size();
    for (uint32_t k = 0; k < h.n_cigar; k++) { const uint32_t len = (uint32_t)num(), op = (uint32_t)num(); S.cigar.push_back(len << 4 | op); }
    S.hdr.push_back(h); S.name_hash.push_back(name);
  }
  fclose(f);
  try {
    ShardPlan pl;
    const PlanInput in{S, T, layouts, cc, n_focus != 0, focus, combos, iv_starts, false, 0, hemi_iv, tile_positions, 0, wp, PlanKnobs()};
    find_shared_names(in, pl);
    build_params(in, pl);
    class_ids(S, T, &pl.class_list, pl.n_class, true);
    flag_sum_errors(in, pl);
    layout_event_slices(in, pl);
    check_sorted_and_depth(in, pl);
    plan_tiles(in, pl);
    candidate_reads(in, pl);
    plan_name_owners(in, pl, [](uint32_t) -> std::vector<uint32_t> { throw Error(MKP_E_DEVICE, "no device here"); });
    split_fused_and_cover(in, pl);
    build_work_records(in, pl);
    printf("plan stream %d wide %d slot_cap %u n_tiles %u cov_bytes %" PRIu64 " events_cap %" PRIu64 " groups %zu\n", (int)pl.stream, (int)pl.wide,
        pl.slot_cap, pl.n_tiles, pl.cov_bytes, (uint64_t)S.n_events_cap, pl.dup_groups.size());
    for (size_t i = 0; i < n; i++) printf("read %zu %u %u %u %u %d\n", i, S.hdr[i].gs0, S.hdr[i].n_sl, S.hdr[i].cov_off, S.hdr[i].event_off,
        (int)pl.dup_member[i]);
    for (auto& t : pl.tiles) printf("tile %d %d %u %u\n", t.r0, t.r1, t.first, t.last);
    for (auto& t : pl.stiles) printf("stile %u %u %u %u %d %d %u %u\n", t.g0, t.g1, t.gh0, t.gh1, t.r0, t.r1, t.first, t.last);
    for (auto& d : pl.dup_cons) printf("cons %u %u %u %u %u %u\n", d.rid, d.seg_off, d.n_seg, d.own_off, d.eff_off, d.eff_cap);
    for (auto& s : pl.dup_segs) printf("seg %d %d %u %u\n", s.p_lo, s.p_hi, s.src_off, s.owner);
  } catch (const Error& e) {
    printf("error %d %s\n", e.status, e.what());
  }
  return 0;
}
