// The reads sampler's schedule as plain arithmetic: which contig gets how many reads, which intervals form a super batch, how a contig's quota
// spreads over them (sampling_schedule.rs:171-615, interval_chunks.rs:563-643), the per-interval quotas of `extract calls --num-reads` and the
// rank that owns a sampling interval.  No device, no BAM: contigs come in as anything with {tid, start, length, end()} (Target, or the
// driver's Contig), index counts as IdxStats (the driver's idxstats() reads them from the BAM index).  Every float / double / ceilf / ceil and cast mirrors the reference's types: the parity tests
// are bit-exact.  tests/sample_schedule_host.cpp runs these functions alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <vector>

namespace mkp {

// a schedule that cannot be made (the driver reports it as MKP_E_THRESHOLD)
struct ScheduleRefusal : std::runtime_error { using std::runtime_error::runtime_error; };

struct IdxStats { std::map<int64_t, uint64_t> mapped_by_tid; uint64_t mapped = 0, unmapped = 0; };
struct Quota { bool all = false; size_t n = 0; };
struct Iv { uint32_t tid, start, end; };
struct SampleIv { Iv iv; Quota q; };
struct Target { uint32_t tid, start, length; uint32_t end() const { return start + length; } };   // a target record (or a region of one)

// SamplingSchedule::from_num_reads (sampling_schedule.rs:171-273): per contig ceil(N * its share of the reads), capped by its count; while the
// sum overshoots N by more than half, contigs at or under a rising floor are dropped (the reference walks an FxHashMap there; ascending tid
// here — order unpinned)
inline std::map<uint32_t, Quota> quota_from_num_reads(const IdxStats& st, size_t num_reads, bool include_unmapped) {
  const uint64_t total_u = include_unmapped ? st.mapped + st.unmapped : st.mapped;
  if (total_u == 0) throw ScheduleRefusal("zero reads found in bam index");
  std::map<uint32_t, Quota> quota;
  const float total = (float)total_u; size_t sum = 0;
  for (auto& kv : st.mapped_by_tid) if (kv.second) { Quota q;
    q.n = std::min<size_t>((size_t)ceilf((float)num_reads * ((float)kv.second / total)), (size_t)kv.second);
    sum += q.n; quota[(uint32_t)kv.first] = q; }
  if (include_unmapped) sum += (size_t)ceilf((float)num_reads * ((float)st.unmapped / total));
  size_t floor = 1;
  while ((double)sum / (double)num_reads > 1.5) {
    for (auto& kv : quota) { if (kv.second.n <= floor) { sum -= kv.second.n; kv.second.n = 0; } if (sum <= num_reads) break; }
    sum = 0; for (auto& kv : quota) sum += kv.second.n; floor++;
  }
  for (auto it = quota.begin(); it != quota.end();) { if (!it->second.all && it->second.n == 0) it = quota.erase(it); else ++it; }
  return quota;
}

// SamplingSchedule::from_sample_frac (sampling_schedule.rs:321-381): every contig with reads gets ceil(count * f), or all of them at f == 1
inline std::map<uint32_t, Quota> quota_from_sample_frac(const IdxStats& st, double sampling_frac) {
  std::map<uint32_t, Quota> quota;
  const float f = (float)sampling_frac;
  for (auto& kv : st.mapped_by_tid) if (kv.second) { Quota q; if (f == 1.0f) q.all = true; else q.n = (size_t)ceilf((float)kv.second * f);
      quota[(uint32_t)kv.first] = q; }
  return quota;
}

// ReferenceIntervalsFeeder (interval_chunks.rs:563-643): the targets cut into intervals of `interval_size`, collected into groups
// (MultiChromCoordinates, in feeder order) that run across contigs until they hold an interval's worth of bases
template <class C> std::vector<std::vector<Iv>> feeder_groups(const std::vector<C>& contigs, uint32_t interval_size) {
  std::vector<std::vector<Iv>> groups;
  std::vector<Iv> batch; uint32_t blen = 0;
  for (auto& c : contigs) for (uint32_t p = c.start; p < c.end();) {
    uint32_t e = (uint32_t)std::min<uint64_t>((uint64_t)p + interval_size, c.end());
    batch.push_back({c.tid, p, e}); blen += e - p;
    if (blen >= interval_size) { groups.push_back(batch); batch.clear(); blen = 0; }
    p = e; }
  if (!batch.empty()) groups.push_back(batch);
  return groups;
}

// the feeder over the sampling grid: the intervals of every super-batch of `batch_size` feeder groups, by contig and start
template <class C> std::vector<std::vector<Iv>> sampling_super_batches(const std::vector<C>& contigs, uint32_t interval_size, size_t batch_size) {
  const std::vector<std::vector<Iv>> groups = feeder_groups(contigs, interval_size);
  std::vector<std::vector<Iv>> out;
  for (size_t g0 = 0; g0 < groups.size(); g0 += std::max<size_t>(batch_size, 1)) {
    std::vector<Iv> all;
      for (size_t g = g0; g < std::min(groups.size(), g0 + std::max<size_t>(batch_size, 1)); g++) for (auto& iv : groups[g]) all.push_back(iv);
    std::stable_sort(all.begin(), all.end(), [](const Iv& x, const Iv& y) { return x.tid != y.tid ? x.tid < y.tid : x.start < y.start; });
    out.push_back(std::move(all));
  }
  return out;
}

// accumulate_sample_counts (sampling_schedule.rs:440-615): the intervals of one super-batch with their quotas — what is left of each contig's
// quota spread over its intervals by length, intervals whose share is under 50 reads merged with their neighbours
inline std::vector<SampleIv> group_super_batch(const std::vector<Iv>& all, const std::map<uint32_t, uint32_t>& contig_size,
    const std::map<uint32_t, Quota>& quota, const std::map<uint32_t, size_t>& sampled_so_far) {
  std::map<uint32_t, uint32_t> len_per; for (auto& iv : all) len_per[iv.tid] += iv.end - iv.start;
  std::map<uint32_t, Quota> per_chrom;
  for (auto& kv : len_per) { auto cs = contig_size.find(kv.first); auto q = quota.find(kv.first);
    if (cs == contig_size.end() || q == quota.end()) continue;
      auto sf = sampled_so_far.find(kv.first); size_t so_far = sf != sampled_so_far.end() ? sf->second : 0;
      float f = (float)kv.second / (float)cs->second;
    if (q->second.all) per_chrom[kv.first] = q->second; else if (q->second.n > so_far) { Quota x;
      x.n = (size_t)ceilf(f * (float)(q->second.n - so_far));
        per_chrom[kv.first] = x; } }
  std::vector<SampleIv> grouped; bool have_slack = false; Iv slack{0, 0, 0}; size_t slack_n = 0;
  auto merged = [](const Iv& x, const Iv& y) { return Iv{x.tid, std::min(x.start, y.start), std::max(x.end, y.end)}; };
  for (auto& iv : all) {
    auto pc = per_chrom.find(iv.tid); if (pc == per_chrom.end()) continue;
    if (pc->second.all) { grouped.push_back({iv, pc->second}); continue; }
    float f = (float)(iv.end - iv.start) / (float)len_per[iv.tid]; size_t x = (size_t)ceilf((float)pc->second.n * f); Quota qx; qx.n = x;
    if (x < 50) {
      if (have_slack) { if (slack.tid == iv.tid) { Iv m = merged(slack, iv); size_t tot = x + slack_n; if (tot < 50) { slack = m; slack_n = tot;
          } else { Quota q;
          q.n = tot; grouped.push_back({m, q}); have_slack = false; } } else { Quota q; q.n = slack_n; grouped.push_back({slack, q}); slack = iv;
            slack_n = x; } }
      else { have_slack = true; slack = iv; slack_n = x; }
    } else if (have_slack) { have_slack = false; if (slack.tid == iv.tid) { Quota q; q.n = slack_n + x; grouped.push_back({merged(slack, iv), q});
      } else { Quota q;
        q.n = slack_n; grouped.push_back({slack, q}); grouped.push_back({iv, qx}); } }
    else grouped.push_back({iv, qx});
  }
  if (have_slack) { Quota q; q.n = slack_n; grouped.push_back({slack, q}); }
  return grouped;
}

// `extract calls --num-reads` on an indexed BAM (get_record_sampler, sampling_schedule.rs:417-438): every interval of the feeder has a
// RecordSampler of its own, ceil(contig quota * interval length / length of the whole super batch) records; a super batch is `batch_size`
// feeder groups.  Per contig the feeder's intervals, ascending and disjoint.
struct IvQuota { uint32_t start, end; long nr; long used; };   // nr == -2: the schedule holds nothing for the contig (never fetched)
inline std::map<uint32_t, std::vector<IvQuota>> extract_interval_quotas(const std::vector<std::vector<Iv>>& groups, size_t batch_size,
    const std::map<uint32_t, Quota>& quota) {
  std::map<uint32_t, std::vector<IvQuota>> iv_quota;
  for (size_t g0 = 0; g0 < groups.size(); g0 += batch_size) {
    uint64_t total_len = 0;
    for (size_t g = g0; g < std::min(groups.size(), g0 + batch_size); g++) for (auto& iv : groups[g]) total_len += iv.end - iv.start;
    for (size_t g = g0; g < std::min(groups.size(), g0 + batch_size); g++) for (auto& iv : groups[g]) {
      auto q = quota.find(iv.tid);
      const long nr = q == quota.end() ? 0 /* chrom_has_reads: never fetched */
          : (long)std::ceil((double)q->second.n * ((double)(iv.end - iv.start) / (double)(uint32_t)total_len));
      iv_quota[iv.tid].push_back({iv.start, iv.end, q == quota.end() ? -2 : nr, 0});
    }
  }
  return iv_quota;
}

// The sampling grid of a rank-sharded estimate: the scheduled contigs laid end to end.  An interval belongs to the rank whose contiguous run
// of the grid, by base pairs, holds its midpoint (as the pileup shards are dealt).
struct SamplingGrid {
  std::map<uint32_t, uint64_t> base, start; uint64_t bp = 0;   // per contig: its offset in the grid, its first position; the grid's length
  SamplingGrid() = default;
  template <class C> explicit SamplingGrid(const std::vector<C>& contigs) { for (auto& c : contigs) { base[c.tid] = bp; start[c.tid] = c.start; bp += c.length; } }
  uint32_t owner(const Iv& iv, uint32_t world) const {
    const uint64_t mid = base.at(iv.tid) + (iv.start - start.at(iv.tid)) + (iv.end - iv.start) / 2;
    return (uint32_t)std::min<uint64_t>(world - 1, mid * world / std::max<uint64_t>(bp, 1));
  }
};

}  // namespace mkp
