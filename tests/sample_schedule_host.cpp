// Host program of tests/test_sample_schedule_host.py: the reads sampler's schedule (modkit_amd/csrc/mkp_sample_schedule.hpp) alone — no BAM,
// no device.  Reads one scenario as whitespace-separated words, the first one naming the function:
//   quota   num_reads include_unmapped unmapped n (tid mapped)..
//   frac    fraction n (tid mapped)..
//   batches interval_size batch_size n (tid start length)..
//   group   n (tid start end)..  n (tid contig_size)..  n (tid all quota)..  n (tid sampled_so_far)..
//   extract interval_size batch_size n (tid start length)..  n (tid quota)..
//   owner   world interval_size n (tid start length)..
// and prints what the function made, one item per line; a refusal is printed as `error <message>`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "mkp_sample_schedule.hpp"

using namespace mkp;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r"); if (!f) return 2;
  auto num = [&]() { long long v = 0; if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short scenario\n"); exit(2); } return v; };
  auto targets = [&]() { std::vector<Target> c((size_t)num());
    for (auto& t : c) { t.tid = (uint32_t)num(); t.start = (uint32_t)num(); t.length = (uint32_t)num(); } return c; };
  auto counts = [&](IdxStats* st) { const size_t n = (size_t)num();
    for (size_t k = 0; k < n; k++) { const int64_t tid = num(); const uint64_t m = (uint64_t)num(); st->mapped_by_tid[tid] = m; st->mapped += m; } };
  auto print_quota = [](const std::map<uint32_t, Quota>& q) {
    for (auto& kv : q) { if (kv.second.all) printf("quota %u all\n", kv.first); else printf("quota %u %zu\n", kv.first, kv.second.n); } };
  char what[16]; if (fscanf(f, "%15s", what) != 1) return 2;
  const std::string w = what;
  try {
    if (w == "quota") {
      const size_t n_reads = (size_t)num(); const bool unmapped = num() != 0; IdxStats st; st.unmapped = (uint64_t)num(); counts(&st);
      print_quota(quota_from_num_reads(st, n_reads, unmapped));
    } else if (w == "frac") {
      double frac = 0; if (fscanf(f, "%lf", &frac) != 1) return 2;
      IdxStats st; counts(&st); print_quota(quota_from_sample_frac(st, frac));
    } else if (w == "batches") {
      const uint32_t interval = (uint32_t)num(); const size_t batch = (size_t)num();
      size_t k = 0;
      for (auto& all : sampling_super_batches(targets(), interval, batch)) { for (auto& iv : all) printf("iv %zu %u %u %u\n", k, iv.tid, iv.start, iv.end);
        k++; }
    } else if (w == "group") {
      std::vector<Iv> all((size_t)num()); for (auto& iv : all) { iv.tid = (uint32_t)num(); iv.start = (uint32_t)num(); iv.end = (uint32_t)num(); }
      std::map<uint32_t, uint32_t> size; for (size_t n = (size_t)num(); n > 0; n--) { const uint32_t t = (uint32_t)num(); size[t] = (uint32_t)num(); }
      std::map<uint32_t, Quota> quota; for (size_t n = (size_t)num(); n > 0; n--) { const uint32_t t = (uint32_t)num(); Quota q; q.all = num() != 0;
        q.n = (size_t)num(); quota[t] = q; }
      std::map<uint32_t, size_t> so_far; for (size_t n = (size_t)num(); n > 0; n--) { const uint32_t t = (uint32_t)num(); so_far[t] = (size_t)num(); }
      for (auto& g : group_super_batch(all, size, quota, so_far)) { if (g.q.all) printf("giv %u %u %u all\n", g.iv.tid, g.iv.start, g.iv.end);
        else printf("giv %u %u %u %zu\n", g.iv.tid, g.iv.start, g.iv.end, g.q.n); }
    } else if (w == "extract") {
      const uint32_t interval = (uint32_t)num(); const size_t batch = (size_t)num();
      const std::vector<Target> c = targets();
      std::map<uint32_t, Quota> quota; for (size_t n = (size_t)num(); n > 0; n--) { const uint32_t t = (uint32_t)num(); quota[t].n = (size_t)num(); }
      for (auto& kv : extract_interval_quotas(feeder_groups(c, interval), batch, quota)) for (auto& q : kv.second)
        printf("ivq %u %u %u %ld\n", kv.first, q.start, q.end, q.nr);
    } else if (w == "owner") {
      const uint32_t world = (uint32_t)num(), interval = (uint32_t)num();
      const std::vector<Target> c = targets(); const SamplingGrid grid(c);
      for (auto& all : sampling_super_batches(c, interval, 1)) for (auto& iv : all) printf("owner %u %u %u %u\n", iv.tid, iv.start, iv.end,
          grid.owner(iv, world));
    } else return 2;
  } catch (const ScheduleRefusal& e) { printf("error %s\n", e.what()); }
  fclose(f);
  return 0;
}
