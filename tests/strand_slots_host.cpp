// Host program of tests/test_strand_slots_host.py: the planner's slot-entry lists and the fused reads' runs in them
// (modkit_amd/csrc/mkp_plan.hpp: window_slots, plan_read_entries, build_work_records) on read headers written by hand — no BAM records, no
// device.  Reads a scenario as whitespace-separated numbers:
//   win_start win_end
//   n_focus, then per focus position: position rule          (rule: 1 '+', 2 '-', 3 both)
//   n_reads, then per read: ref_start ref_end reverse tags   (tags: 0 `C+m?`, 1 `C-m?` — the mod strand sg0 = 1 —, 2 no MM tag at all)
// runs the planner's stages in their order (the knobs come from the environment, as in the library) and prints the three lists and
// every work record as text; a refusal is printed as `error <status> <message>`.
#include <cinttypes>
#include <cstdio>

#include "mkp_plan.hpp"

using namespace mkp;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r"); if (!f) return 2;
  auto num = [&]() { long long v = 0; if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short scenario\n"); exit(2); } return v; };
  ShardHost S; LayoutTables T; CallerCfg cc; WindowPlan wp;
  std::vector<LayoutHost> layouts(2);
  for (int sg = 0; sg < 2; sg++) { TagHeader t; t.fb = 1; t.neg = sg != 0; t.mode = 0; t.codes = {(uint32_t)'m'}; layouts[(size_t)sg].tags.push_back(t); }
  S.win_start = (int32_t)num(); S.win_end = (int32_t)num();
  PodVec<uint8_t> focus; std::vector<mkp_motif_combo> combos;
  focus.assign((size_t)(S.win_end - S.win_start), 0);
  const size_t n_focus = (size_t)num();
  for (size_t k = 0; k < n_focus; k++) { const long long p = num(), rule = num(); focus[(size_t)(p - S.win_start)] = (uint8_t)(rule & 3); }
  { mkp_motif_combo z; memset(&z, 0, sizeof(z)); combos.push_back(z); }
  std::vector<uint32_t> iv_starts, hemi_iv;
  const size_t n = (size_t)num();
  for (size_t i = 0; i < n; i++) {
    MkpReadHdr h; memset(&h, 0, sizeof(h));
    h.ref_start = (int32_t)num(); h.ref_end = (int32_t)num(); h.l_seq = (uint32_t)(h.ref_end - h.ref_start); h.event_cap = 4;
    if (num()) h.flags |= MKP_RF_REVERSE;
    const long long tags = num();
    h.n_cigar = 1; h.cigar_off = (uint32_t)S.cigar.size(); S.cigar.push_back(h.l_seq << 4);
    h.tag_off = (uint32_t)S.tagref.size();
    if (tags < 2) { h.n_tags = 1; h.layout = (uint16_t)tags; MkpTagRef t; memset(&t, 0, sizeof(t)); t.n = 1; S.tagref.push_back(t); }
    S.hdr.push_back(h); S.name_hash.push_back(0x1000000000000000ull + 16ull * i);
  }
  fclose(f);
  try {
    ShardPlan pl;
    const PlanInput in{S, T, layouts, cc, true, focus, combos, iv_starts, false, 0, hemi_iv, 0, 0, wp, PlanKnobs::from_env()};
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
    const SlotLists& L = pl.lists;
    printf("lists %u %u %u %zu %" PRIu64 " %" PRIu64 "\n", L.n_all, L.n_strand[0], L.n_strand[1], L.ent.size(), pl.fused_entries, pl.fused_slots);
    for (auto& e : L.ent) printf("ent %u %u\n", e.pos, e.g);
    for (size_t g = 0; g < L.rank[0].size(); g++) printf("rank %u %u\n", L.rank[0][g], L.rank[1][g]);
    for (auto& w : pl.work) printf("work %u %u %u %u %u %u\n", w.rid, w.gs0, w.n_sl, w.cov_off, w.ent_off, w.n_ent);
    for (size_t k = pl.n_slot_class[0]; k < pl.slot_ids.size(); k++) printf("cover %u\n", pl.slot_ids[k]);
  } catch (const Error& e) {
    printf("error %d %s\n", e.status, e.what());
  }
  return 0;
}
