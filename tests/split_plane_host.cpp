// Host program of tests/test_split_plane_host.py: the planner's stage that lays the fused reads into the call plane and the base plane and
// counts what a pass reads of them (build_work_records, plane_lookup_bytes: modkit_amd/csrc/mkp_plan.hpp) — no BAM records, no device.
// Reads whitespace-separated numbers:
//   n_reads, then per read: l_seq n_ent flags n_tags calls_of_tag0 calls_of_tag1 n_cigar
//   n_queries, then per query: l_seq n_ent with_calls n_calls
// Every read is a fused read, in the order given (the launch order), with n_ent slot entries.  Prints per read `work k pad n_calls`, then
// `plan plane_bytes B looked_up B swept B entries N`, then per query `bound value`.
#include <cinttypes>
#include <cstdio>

#include "mkp_plan.hpp"

using namespace mkp;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r"); if (!f) return 2;
  auto num = [&]() { long long v = 0; if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short scenario\n"); exit(2); } return v; };
  ShardHost S; LayoutTables T; std::vector<LayoutHost> layouts; CallerCfg cc; WindowPlan wp;
  PodVec<uint8_t> focus; std::vector<mkp_motif_combo> combos; std::vector<uint32_t> iv_starts, hemi_iv;
  ShardPlan pl;
  const size_t n = (size_t)num();
  uint32_t ent = 0, rank = 0, ml = 0;
  for (size_t i = 0; i < n; i++) {
    MkpReadHdr h; memset(&h, 0, sizeof(h));
    h.l_seq = (uint32_t)num(); const uint32_t n_ent = (uint32_t)num(); h.flags = (uint32_t)num(); h.n_tags = (uint16_t)num();
    const uint32_t calls[2] = {(uint32_t)num(), (uint32_t)num()};
    h.n_cigar = (uint32_t)num(); h.n_sl = 2u * n_ent; h.tag_off = (uint32_t)S.tagref.size();
    for (uint32_t t = 0; t < h.n_tags && t < 2u; t++) {
      MkpTagRef r; memset(&r, 0, sizeof(r)); r.rank_off = rank; r.n = calls[t]; r.ml_off = ml; rank += calls[t]; ml += calls[t];
      S.tagref.push_back(r);
    }
    S.hdr.push_back(h);
    pl.slot_ids.push_back((uint32_t)i); pl.ent_off.push_back(ent); pl.ent_cnt.push_back(n_ent); ent += n_ent;
  }
  pl.stream = true; pl.n_slot_class[0] = (uint32_t)n;
  try {
    const PlanInput in{S, T, layouts, cc, true, focus, combos, iv_starts, false, 0, hemi_iv, 0, 0, wp, PlanKnobs()};
    build_work_records(in, pl);
  } catch (const Error& e) { printf("error %d %s\n", (int)e.status, e.what()); return 0; }
  for (size_t k = 0; k < n; k++) printf("work %zu %u %u\n", k, pl.work[k].pad, pl.work[k].n_calls);
  printf("plan plane_bytes %" PRIu64 " looked_up %" PRIu64 " swept %" PRIu64 " entries %" PRIu64 "\n", pl.plane_bytes, pl.fused_looked_up,
      pl.fused_swept, pl.fused_entries);
  const size_t nq = (size_t)num();
  for (size_t i = 0; i < nq; i++) {
    const uint32_t l_seq = (uint32_t)num(), n_ent = (uint32_t)num(); const bool with_calls = num() != 0; const uint32_t n_calls = (uint32_t)num();
    printf("bound %" PRIu64 "\n", plane_lookup_bytes(l_seq, n_ent, with_calls, n_calls));
  }
  fclose(f);
  return 0;
}
