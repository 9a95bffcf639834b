// `modkit pileup` as a library call: mkp_pileup_main mirrors ModBamPileup::run
// (src/pileup/subcommand.rs:382-816) — same flags, same option resolution, same bedMethyl text —
// with process_region_batch replaced by shards on the GPU.  Host work here is scheduling only:
// BAM ingest, the interval grid + focus positions, choosing which reads the threshold sampler takes
// (reads_sampler/*, sampling_schedule.rs), and formatting rows (writers.rs:87-156).
#include <sys/stat.h>

#include <cerrno>
#include <condition_variable>
#include <deque>
#include <future>
#include <memory>
#include <mutex>
#include <set>
#include <unordered_set>
#include <thread>

#include <unistd.h>

#include "mkp_ctx.hpp"
#include "mkp_dmr.hpp"
#include "mkp_dmr_reps.hpp"
#include "mkp_dmr_sites.hpp"
#include "mkp_ingest_host.hpp"
#include "mkp_focus.hpp"
#include "mkp_regions.hpp"
#include "mkp_bedmethyl_in.hpp"
#include "mkp_writer.hpp"
#include "mkp_rand.hpp"
#include "mkp_sample_schedule.hpp"

using namespace mkp;

namespace {

std::string f32_display(float v);   // (Rust's `{}` of an f32; defined with the extract-calls writer below)

// --bedgraph (BedGraphWriter, writers.rs:264-381): one file per (partition key, strand, mod code[, motif]) in the output directory,
// `[<prefix>_][<key>_]<code>[_<motif label without commas>]_<positive|negative|combined>.bedgraph`, rows
// `chrom <tab> pos <tab> pos + 1 <tab> fraction_modified <tab> filtered_coverage` with the fraction as an f32 through `{}`
// (n_modified as f32 / filtered_coverage as f32, pileup/mod.rs:327-331).  A projection of the bedMethyl rows: same rows, same order per file.
struct BedGraphOut {
  std::string dir, prefix; bool groupings = false; std::vector<std::string> labels; uint64_t n = 0;
  struct File { FILE* f = nullptr; std::string buf; };
  std::map<std::string, File> files;
  void write(const std::string& chrom, const mkp_rows& r) {
    char line[160];
    for (uint64_t i = 0; i < r.n_rows; i++) {
      std::string name;
      if (!prefix.empty()) name = prefix + "_";
      if (groupings) { const uint32_t k = r.partition_key ? r.partition_key[i] : 0u;
        name += (k < r.n_partition_keys ? r.partition_key_names[k] : "not_found"); name += "_"; }
      const uint32_t code = r.code_repr[i];
      if (code & 0x80000000u) name += std::to_string(code & 0x7fffffffu); else name += (char)code;
      if (r.motif_idx[i] >= 0 && (size_t)r.motif_idx[i] < labels.size()) { name += "_";
        for (char ch : labels[(size_t)r.motif_idx[i]]) if (ch != ',') name += ch;
        }
      name += r.strand[i] == '+' ? "_positive" : r.strand[i] == '-' ? "_negative" : r.strand[i] == '.' ? "_combined" : "__unknown";
      File& fl = files[name];
      if (!fl.f) { const std::string path = dir + "/" + name + ".bedgraph"; fl.f = fopen(path.c_str(), "w");
        if (!fl.f) throw Error(MKP_E_IO, "failed to make output file " + path);
        }
      const float frac = (float)r.n_mod[i] / (float)r.n_valid[i];
      const int k = snprintf(line, sizeof(line), "\t%u\t%u\t%s\t%u\n", r.pos[i], r.pos[i] + 1, f32_display(frac).c_str(), r.n_valid[i]);
      fl.buf += chrom; fl.buf.append(line, (size_t)k);
      if (fl.buf.size() > ((size_t)1 << 20)) {
        if (fwrite(fl.buf.data(), 1, fl.buf.size(), fl.f) != fl.buf.size()) throw Error(MKP_E_IO, "write error in " + dir);
        fl.buf.clear(); }
      n++;
    }
  }
  void finish() { for (auto& kv : files) { File& fl = kv.second; if (fl.f) {
        if (!fl.buf.empty() && fwrite(fl.buf.data(), 1, fl.buf.size(), fl.f) != fl.buf.size()) throw Error(MKP_E_IO, "write error in " + dir);
        fclose(fl.f); fl.f = nullptr; } } }
  ~BedGraphOut() { for (auto& kv : files) if (kv.second.f) fclose(kv.second.f); }
};

struct Args {
  std::string in_bam, out_bed, region, sample_region, include_bed, ignore, ref_fasta, edge_filter, preset;
  uint32_t max_depth = 8000, interval_size = 100000, sampling_interval_size = 1000000;
  bool have_seed = false; uint64_t seed = 0;   // --seed
  bool serial_sampler = false;   // sample-probs / summary / extract calls on a BAM that has no index file (reads_sampler/mod.rs:129-158)
  size_t threads = 4, num_reads = 10042; bool have_frac = false; double sampling_frac = 0; bool no_filtering = false; float filter_percentile = 0.1f;
  std::vector<std::string> filter_threshold, mod_thresholds, motif_parts, partition_tags; std::string prefix;
  bool include_unmapped = false, force_allow = false, cpg = false, mask = false, combine_mods = false, combine_strands = false, invert_edge = false,
      mixed_delim = false, with_header = false;
  int device = 0; uint32_t rank = 0, world = 1;
      uint64_t shard_bp = 0,
          shard_bytes = 256ull << 20 /* BAM bytes per shard (indexed input): bounds host memory, and the next shard inflates while this one is packed and run */;
      bool no_index = false; uint32_t tile = 0; bool stats = false, plan_only = false; uint32_t rerun = 0, plan_pack_min = 1024;
  bool hemi = false;   /* `pileup-hemi` (DuplexModBamPileup, subcommand.rs:827-1514) */
  mkp_threshold_fn thr_cb = nullptr; void* thr_cb_user = nullptr;
    /* mkp_pileup_run_cb: the pass thresholds come from the caller (multi-GPU: all-reduced histograms / a broadcast) */
  uint64_t hbm_budget_mb = 0;   /* --hbm-budget-mb: device memory the shards ingested ahead may hold (0: 55 % of the device) */
  bool device_inflate = false;
    /* inflate the shards' BGZF windows on the GPU (mkp_inflate_wave4.hip) instead of the host pool, records back to the host packer */
  bool host_ingest = false, shard_bytes_set = false;
    /* --host-ingest (or MKP_HOST_INGEST=1): inflate, cut and pack the shards on the host instead of the device (mkp_ingest.hip) */
  bool bedgraph = false;
    /* --bedgraph: the output path is a directory of <code>[_<motif>]_<strand>.bedgraph files (BedGraphWriter, writers.rs:264-381) */
  bool bgzf = false;   /* write the bedMethyl as BGZF + a .tbi index (what `bgzip` + `tabix -p bed` make of the reference's output) */
  /* --region-stats <bed>: `modkit stats` over this run's rows, reduced on the device from the rows in HBM (mkp_stats.hip); the table goes to
     --region-stats-out; --region-stats-codes / -min-coverage / -no-header = its --mod-codes / --min-coverage / --no-header;
     --region-stats-only: the rows are neither read back nor written (the out.bed positional is not created) */
  std::string region_stats, region_stats_out; std::vector<uint32_t> region_stats_codes; uint64_t region_stats_min_cov = 1;
  bool region_stats_no_header = false, region_stats_only = false;
  /* --localize <bed>: `modkit localize` over this run's rows, an offset histogram built on the device from the rows in HBM
     (mkp_localize.hip), contig lengths from the BAM header; the table goes to --localize-out; --localize-window / -stranded /
     -stranded-features = its --window / --stranded / --stranded-features; --localize-only: as --region-stats-only */
  std::string localize, localize_out; uint32_t localize_window = 2000; bool have_localize_window = false;
  int localize_stranded = 0, localize_stranded_features = 0; bool localize_only = false;
  /* --merge-bedmethyl <prior.bed> (repeatable): the output is `bedmethyl merge` of this run's rows with the prior tables (plain text or bgzip),
     joined on the device from the rows in HBM (mkp_merge.hip); contig lengths and order from the BAM header */
  std::vector<std::string> merge_bedmethyl;
  bool rows_stay() const { return region_stats_only || localize_only; }   // the rows are neither read back nor written
};

struct RegionSpec { std::string name; uint32_t start, end; };

uint64_t peak_rss_kb() {   // VmHWM of this process (--stats)
  std::ifstream f("/proc/self/status"); std::string line;
  while (std::getline(f, line)) if (line.compare(0, 6, "VmHWM:") == 0) return strtoull(line.c_str() + 6, nullptr, 10);
  return 0;
}

RegionSpec parse_region(const std::string& raw, const BamSource& bam) {  // Region::parse_str (util.rs:463-524)
  auto bad = [&]() { return Error(MKP_E_INVALID, "invalid region, " + raw + ", should be 'chrom' or 'chrom:start-stop'"); };
  size_t c = raw.find(':');
  if (c == std::string::npos) { int tid = bam.tid_of(raw); if (tid < 0) throw Error(MKP_E_INVALID, "contig-missing");
    return {raw, 0, bam.ref_lens[(size_t)tid]}; }
  if (raw.find(':', c + 1) != std::string::npos) throw bad();
  std::string se = raw.substr(c + 1); std::vector<uint32_t> v; size_t s = 0;
  for (;;) { size_t d = se.find('-', s); std::string part = se.substr(s, d == std::string::npos ? std::string::npos : d - s), cl;
      for (char ch : part) if (ch != ',') cl += ch; if (cl.empty()) throw bad(); uint64_t x = 0; for (char ch : cl) {
        if (ch < '0' || ch > '9') throw bad();
      x = x * 10 + (uint64_t)(ch - '0'); if (x > 0xffffffffull) throw bad(); } v.push_back((uint32_t)x); if (d == std::string::npos) break; s = d + 1;
        }
  if (v.size() != 2 || v[1] <= v[0]) throw bad();
  return {raw.substr(0, c), v[0], v[1]};
}

bool parse_code(const std::string& s, uint32_t* out) {  // ModCodeRepr::parse (mod_base_code.rs:112-122)
  if (s.size() == 1) { *out = (uint32_t)(unsigned char)s[0]; return true; }
  if (s.empty()) return false;
  uint64_t v = 0; for (char c : s) { if (c < '0' || c > '9') return false; v = v * 10 + (uint64_t)(c - '0'); if (v > 0x7fffffffull) return false; }
  *out = 0x80000000u | (uint32_t)v; return true;
}

std::vector<Contig> targets(const BamSource& bam, const RegionSpec* r) {  // get_targets (util.rs:409-446)
  std::vector<Contig> out;
  for (size_t t = 0; t < bam.ref_names.size(); t++) { if (r) {
      if (bam.ref_names[t] == r->name) out.push_back({(uint32_t)t, r->start, r->end - r->start,
      bam.ref_names[t]}); } else out.push_back({(uint32_t)t, 0, bam.ref_lens[t], bam.ref_names[t]}); }
  return out;
}

IdxStats idxstats(const BamSource& bam, const RegionSpec* region, const BedFilter* bf) {  // IdxStats::new_from_reader (sampling_schedule.rs:649-716)
  IdxStats st; int rt = region ? bam.tid_of(region->name) : -1;
  if (region && rt < 0) throw Error(MKP_E_INVALID, "did not find target_id for region");
  std::vector<uint64_t> m, u; uint64_t nocoor = 0;
  bam.counts(&m, &u, &nocoor);   // the index's per-reference counts (htslib idxstats), or a count over the resident file
  auto keep = [&](int64_t t) { if (region) return t == rt; if (bf) return bf->has_chrom(t); return true; };
  for (size_t t = 0; t < m.size(); t++) if (keep((int64_t)t)) { st.mapped += m[t]; st.unmapped += u[t]; st.mapped_by_tid[(int64_t)t] = m[t]; }
  if (keep(-1)) st.unmapped += nocoor;
  return st;
}

void must(mkp_ctx* ctx, int r) { if (r != MKP_OK) throw Error(r, mkp_last_error(ctx)); }

// The C ABI's epilogues: what a call's body throws becomes its status, the message going into the context (`ctx->err`), into the caller's
// buffer, or nowhere
int fail_into(char* errbuf, size_t errbuf_len, int st, const std::string& m) {
  if (errbuf && errbuf_len) { snprintf(errbuf, errbuf_len, "%s", m.c_str()); } return st; }
template <class F> int guarded_ctx(mkp_ctx* ctx, F body) {
  try { return body(); }
  catch (const Error& e) { ctx->err = e.what(); return e.status; }
  catch (const std::exception& e) { ctx->err = e.what(); return MKP_E_INVALID; }
}
template <class F> int guarded_buf(char* errbuf, size_t errbuf_len, F body) {
  try { return body(); }
  catch (const Error& e) { return fail_into(errbuf, errbuf_len, e.status, e.what()); }
  catch (const std::exception& e) { return fail_into(errbuf, errbuf_len, MKP_E_INVALID, e.what()); }
}
template <class F> int guarded_status(F body) {
  try { return body(); } catch (const Error& e) { return e.status; } catch (const std::exception&) { return MKP_E_INVALID; }
}

// --edge-filter / --invert-edge-filter into the caller config (parse_edge_filter_input, command_utils.rs:243-277)
void parse_edge_filter(const Args& a, mkp_caller* kc) {
  if (a.edge_filter.empty()) return;
  kc->edge_filter = 1; kc->edge_inverted = a.invert_edge; size_t c = a.edge_filter.find(',');
  if (c != std::string::npos) { kc->edge_start = (uint32_t)strtoul(a.edge_filter.c_str(), nullptr, 10);
      kc->edge_end = (uint32_t)strtoul(a.edge_filter.c_str() + c + 1, nullptr, 10); }
  else kc->edge_start = kc->edge_end = (uint32_t)strtoul(a.edge_filter.c_str(), nullptr, 10);
}
// --mod-thresholds <code>:<threshold>
std::vector<mkp_mod_threshold> parse_mod_thresholds(const std::vector<std::string>& raws) {
  std::vector<mkp_mod_threshold> per_mod;
  for (auto& raw : raws) { size_t c = raw.find(':'); uint32_t code;
      if (c == std::string::npos || raw.find(':', c + 1) != std::string::npos || !parse_code(raw.substr(0, c), &code)) throw Error(MKP_E_INVALID,
      "encountered illegal per-mod threshold: " + raw);
      per_mod.push_back({code, strtof(raw.c_str() + c + 1, nullptr)}); }
  return per_mod;
}

struct SampleTimes { double fetch_ms = 0, device_ms = 0, decide_ms = 0; uint64_t rounds = 0, reads = 0; };
SampleTimes g_sample_times;   // --stats: where the threshold estimate's time went (last run in this process)

// the schedule header knows no status codes: its refusal leaves as the threshold error it always was
std::map<uint32_t, Quota> num_reads_quotas(const IdxStats& st, size_t num_reads, bool include_unmapped) {
  try { return quota_from_num_reads(st, num_reads, include_unmapped); } catch (const ScheduleRefusal& e) { throw Error(MKP_E_THRESHOLD, e.what()); }
}

// A read name as the resident shards know it: two 64-bit hashes
struct NameKey { uint64_t a, b; bool operator==(const NameKey& o) const { return a == o.a && b == o.b; } };
struct NameKeyHash { size_t operator()(const NameKey& k) const { return (size_t)(k.a ^ (k.b * 0x9e3779b97f4a7c15ull)); } };
// Records of a resident shard are numbered kept reads first (index < hdr.size(), digest order), then the sampler-only reads (QC-fail ...: few)
NameKey resident_name_key(const ShardHost& S, uint32_t k) {
  const size_t n = S.hdr.size();
  return k < n ? NameKey{S.name_hash[k], S.dev_name_hash2[k]} : NameKey{S.so_name_hash[k - n], S.so_name_hash2[k - n]};
}
// the records of resident shard S that satisfy `pred` — of the kept reads only [first, last) are looked at — in file order: the kept
// records in digest order, the sampler-only records merged in by their place in the file (window index)
template <class Pred> std::vector<uint32_t> resident_ids(const ShardHost& S, size_t first, size_t last, Pred pred) {
  const size_t n = S.hdr.size();
  std::vector<uint32_t> ids; ids.reserve(last - first + S.so_hdr.size());
  for (size_t i = first; i < last; i++) if (pred(S.hdr[i])) ids.push_back((uint32_t)i);
  bool any_so = false;
  for (size_t k = 0; k < S.so_hdr.size(); k++) if (pred(S.so_hdr[k])) { ids.push_back((uint32_t)(n + k)); any_so = true; }
  if (any_so) { auto wi = [&](uint32_t k) { return k < n ? S.dev_win_idx[k] : S.so_win_idx[k - n]; };
    std::stable_sort(ids.begin(), ids.end(), [&](uint32_t x, uint32_t y) { return wi(x) < wi(y); }); }
  return ids;
}

// The records of one fetch as the sampler sees them: a BamBatch of the indexed / whole-file reader, or — `S`: the shard the device ingest
// attached to the context covers the contig — indices into that shard's digest (every kept record is a candidate; names are compared
// through their two 64-bit hashes; the reads' bases and tags are in HBM already, mkp_internal_sample_resident).
struct RecSet {
  // complete: nothing was left out for a later fetch; resident: idx numbers the shard's records as resident_ids does
  std::unique_ptr<BamBatch> b; bool complete = false; const ShardHost* S = nullptr; std::vector<uint32_t> idx;
  size_t size() const { return S ? idx.size() : b->recs.size(); }
  bool truncated(size_t cap) const { return !S && !complete && b->recs.size() >= cap; }
  std::string name(size_t i) const {
    if (S) { const NameKey k = resident_name_key(*S, idx[i]); char key[16]; memcpy(key, &k.a, 8); memcpy(key + 8, &k.b, 8);
      return std::string(key, 16); }
    return b->qname(b->recs[i]);
  }
  int32_t pos(size_t i) const { if (S) { const uint32_t k = idx[i]; const size_t n = S->hdr.size();
      return k < n ? S->hdr[k].ref_start : S->so_hdr[k - n].ref_start; } return b->recs[i].pos; }
  bool candidate(size_t i, bool drop_unmapped) const {
    if (S) return true;
    const BamIndexEntry& e = b->recs[i];
    if ((e.flag & (256 | 1024 | 2048)) || b->l_seq(e) == 0) return false;
    return !(drop_unmapped && (e.flag & 4));
  }
};

// --include-bed: the sampling kernels' per-contig masks (BedFilter::mask), built on first use; none without a BED
struct BedMasks {
  const BedFilter* bf; const BamSource& bam; std::map<uint32_t, std::vector<uint8_t>> by_tid;
  const uint8_t* operator()(uint32_t tid) {
    if (!bf) return nullptr;
    auto it = by_tid.find(tid); if (it == by_tid.end()) it = by_tid.emplace(tid, bf->mask(tid, bam.ref_lens[tid])).first;
    return it->second.data();
  }
};
// the context keeps the device copies of a sampler's BED masks while this object lives: the host masks die with the sampler
struct MaskSession {
  mkp_ctx* c;
  explicit MaskSession(mkp_ctx* ctx) : c(ctx) { mkp_internal_bedmask_reset(c); }
  ~MaskSession() { mkp_internal_bedmask_reset(c); }
};

// what `bam::IndexedReader::from_path` finds (htslib: <bam>.bai, <bam>.csi, or the extension replaced)
bool bam_index_file_exists(const std::string& path) {
  std::vector<std::string> c = {path + ".bai", path + ".csi"};
  if (path.size() > 4 && path.compare(path.size() - 4, 4, ".bam") == 0) { c.push_back(path.substr(0, path.size() - 4) + ".bai");
    c.push_back(path.substr(0, path.size() - 4) + ".csi"); }
  for (auto& f : c) { FILE* p = fopen(f.c_str(), "rb"); if (p) { fclose(p); return true; } }
  return false;
}

// `resident_of` (optional): the device-packed shard holding contig `tid`, bound to the context (mkp_internal_sample_bind) — the estimate then
// samples from HBM; called whenever the schedule moves to another contig.
using ResidentOf = std::function<const ShardHost*(uint32_t tid)>;

// One fetched record set as the first-N logic walks it: the records, `idx` = those that are candidates, `skip` (rank-sharded mode; else
// empty) = the candidates an earlier interval already took
struct Fetched { RecSet set; std::vector<size_t> idx; std::vector<uint8_t> skip; };
// process_records (read_ids_to_base_mod_probs.rs:223-362) over the candidate records of one interval, first-N semantics
struct IntervalState { std::set<std::string> seen; size_t used = 0; };
struct Draws { SeededSampler* rng = nullptr; double frac = 1.0; };   // --sampling-frac < 1: one seeded draw per record (none: every record)
// Default threshold estimation: the reference's deterministic "first N qualifying reads per interval" schedule
// (reads_sampler/mod.rs:30-257, sampling_schedule.rs:171-615); the per-call probabilities come from the decode kernel.
// The values are accumulated in the context's HBM-resident sample (mkp_internal_sample_take); nothing but per-read counts
// comes back to the host.  With --gpus-world W > 1 (full-data mode `-f 1.0` only) a rank walks just its own sampling intervals:
// a read is taken in the first processed interval it overlaps, so the union over ranks is the single-rank sample.
// The stages are the methods, in the order a run meets them.
struct ThresholdSampler {
  using G = SampleIv;
  using Which = std::vector<std::pair<const RecSet*, size_t>>;          // records of a device round: indices into the sets' records, set by set

  mkp_ctx* ctx; const BamSource& bam; const Args& a; const BedFilter* bf; const ResidentOf& resident_of;
  const bool only_mapped, sharded, resident_mode;
  MaskSession mask_session;
  BedMasks bedmask_for;
  SamplingGrid grid;                                        // the scheduled contigs (the owner of an interval; where a contig's grid starts)
  const ShardHost* res = nullptr; uint32_t res_tid = 0xffffffffu;
  std::vector<int32_t> res_pmax;   // resident shard: prefix maximum of the alignment ends (first record that can reach an interval)
  std::set<std::string> taken; std::map<uint32_t, size_t> sampled_so_far;

  ThresholdSampler(mkp_ctx* c, const BamSource& b, const Args& args, const BedFilter* f, const ResidentOf& r)
      : ctx(c), bam(b), a(args), bf(f), resident_of(r), only_mapped(!args.include_unmapped), sharded(args.world > 1), resident_mode((bool)r),
        mask_session(c), bedmask_for{f, b, {}} {}

  // ---- fetch a record set
  void use_contig(uint32_t tid) {   // the shard of contig `tid` becomes the one sampled from
    if (res && res_tid == tid) return;
    res = resident_of(tid); res_tid = tid;
    if (!res || (int32_t)tid != res->tid) throw Error(MKP_E_INVALID, "internal: resident sampling outside the ingested contigs");
    res_pmax.resize(res->hdr.size()); int32_t m = INT32_MIN; for (size_t i = 0; i < res->hdr.size(); i++) {
      m = std::max(m, std::max(res->hdr[i].ref_end, res->hdr[i].ref_start + 1)); res_pmax[i] = m; }
  }
  RecSet fetch_resident(uint32_t tid, uint32_t s, uint32_t e) {
    use_contig(tid);
    RecSet r; r.S = res;
    const size_t first = (size_t)(std::upper_bound(res_pmax.begin(), res_pmax.end(), (int32_t)std::min<uint32_t>(s, 0x7fffffffu)) - res_pmax.begin());
    const size_t last = (size_t)(std::partition_point(res->hdr.begin() + (long)first, res->hdr.end(),
        [&](const MkpReadHdr& h) { return (int64_t)h.ref_start < (int64_t)e; }) - res->hdr.begin());   // (the digest is sorted by start)
    r.idx = resident_ids(*res, first, last, [&](const MkpReadHdr& h) {
      return (int64_t)h.ref_start < (int64_t)e && (int64_t)std::max(h.ref_end, h.ref_start + 1) > (int64_t)s; });
    return r;
  }
  // under --include-bed a read counts only through calls on BED positions (the kernel masks the rest): a read that meets no BED span
  // yields nothing, is not counted and not recorded — so only the records that can meet one are fetched (a sparse BED used to make
  // the estimate inflate every sampling interval whole), all of them: there is no head to extend afterwards.  A record of the interval
  // meets a span inside it, or reaches a span outside it — then it crosses the interval's first or last position.
  RecSet fetch_bed_parts(uint32_t tid, uint32_t s, uint32_t e) const {
    RecSet r; r.b.reset(new BamBatch());
    std::vector<Span> sp = bf->spans_in(tid, s, e);
    sp.push_back({s, (uint64_t)s + 1}); if (e > s + 1) sp.push_back({(uint64_t)e - 1, e});
    std::sort(sp.begin(), sp.end(), [](const Span& x, const Span& y) { return x.s < y.s; });
    merge_spans(sp);
    FetchParts parts; for (auto& x : sp) parts.push_back({(int64_t)x.s, (int64_t)x.e});
    if (!parts.empty()) bam.fetch_parts(tid, parts, r.b.get());
    r.complete = true; return r;
  }
  RecSet fetch(uint32_t tid, uint32_t s, uint32_t e, size_t cap) {
    if (resident_mode) return fetch_resident(tid, s, e);
    if (bf) return fetch_bed_parts(tid, s, e);
    RecSet r; r.b.reset(new BamBatch()); bam.fetch(tid, s, e, r.b.get(), cap); return r;
  }
  static size_t cap_of(const G& g) { return g.q.all ? SIZE_MAX : 2 * g.q.n + 128; }

  // ---- candidates, one device round, the verdict
  Fetched with_candidates(RecSet set, const G* g = nullptr) {   // g: the interval the set was fetched for
    Fetched F; F.set = std::move(set);
    for (size_t i = 0; i < F.set.size(); i++) if (F.set.candidate(i, only_mapped || a.edge_filter.size())) F.idx.push_back(i);
    if (sharded && g) F.skip = skip_list(*g, F);
    return F;
  }
  // decode the records `which` in sampling mode: one device round
  void device_round(const Which& which, uint32_t tid, bool mapped_contig, std::vector<uint32_t>* nv) {
    const uint32_t ws = 0, we = mapped_contig ? bam.ref_lens[tid] : 1; const uint8_t* mask = mapped_contig ? bedmask_for(tid) : nullptr;
    int rc;
    if (resident_mode) { std::vector<uint32_t> ids; ids.reserve(which.size()); for (auto& w : which) ids.push_back(w.first->idx[w.second]);
      rc = mkp_internal_sample_resident(ctx, ws, we, mask, ids.data(), (uint32_t)ids.size(), only_mapped, nv); }
    else { std::vector<mkp_record> recs; recs.reserve(which.size());
      for (auto& w : which) recs.push_back(w.first->b->view(w.first->b->recs[w.second]));
      rc = mkp_internal_sample(ctx, mapped_contig ? (int32_t)tid : -1, ws, we, mask, recs.data(), (uint32_t)recs.size(), only_mapped, nv); }
    must(ctx, rc);
  }
  // the sampler's verdict on candidates F.idx[lo, hi) whose value counts are nv[0 ..): mask[k] = 1 where the read's values enter the sample
  void verdict(const Fetched& F, size_t lo, size_t hi, const uint32_t* nv, long limit, IntervalState* st, uint8_t* mask, Draws draws = Draws()) {
    for (size_t i = lo; i < hi; i++) {
      if (limit >= 0 && st->used >= (size_t)limit) break;   // RecordSampler::ask -> Done
      const size_t k = i - lo;
      if (!F.skip.empty() && F.skip[i]) continue;
      // check_sample_frac (record_sampler.rs:80-86): one draw per record the iterator yields, before anything else is looked at.  Only the
      // unmapped leg and the serial pass draw, and there (the serial pass refuses the filters that could differ) "the tags parse and hold a
      // position" == "a value is left"
      if (draws.rng && nv[k] != 0 && !draws.rng->keep(draws.frac)) continue;    // check_sample_frac -> Skip
      std::string name = F.set.name(F.idx[i]);
      // with_mod_base_info drops reads whose tags fail or are empty before the sampler is asked; a read that parses
      // but keeps no position is asked, not counted, and not recorded
      if (st->seen.count(name)) continue;
      if (nv[k] == 0) continue;
      st->seen.insert(name); st->used++;
      if (taken.count(name)) continue;  // Moniod::op_mut keeps the first occurrence of a read id
      taken.insert(name);
      mask[k] = 1;
    }
  }
  // the candidates of one fetched set from F.idx[from] on, in device rounds until the limit is reached (limit < 0: all of them)
  void take(const Fetched& F, size_t from, long limit, uint32_t tid, bool mapped_contig, IntervalState* st, Draws draws = Draws()) {
    size_t next = from;
    while (next < F.idx.size() && (limit < 0 || st->used < (size_t)limit)) {
      size_t want = limit < 0 ? std::min<size_t>(F.idx.size() - next, 1u << 18) : std::max<size_t>(256, 2 * ((size_t)limit - st->used));
      size_t hi = std::min(F.idx.size(), next + want);
      Which which; which.reserve(hi - next);
        for (size_t i = next; i < hi; i++) which.push_back({&F.set, F.idx[i]});
      std::vector<uint32_t> nv; device_round(which, tid, mapped_contig, &nv);
      std::vector<uint8_t> mask(which.size(), 0);
      verdict(F, next, hi, nv.data(), limit, st, mask.data(), draws);
      must(ctx, mkp_internal_sample_take(ctx, mask));
      next = hi;
    }
  }

  // ---- the intervals of a super batch
  // rank-sharded mode: a read that reaches back into an earlier processed interval of this contig was taken there
  std::vector<uint8_t> skip_list(const G& g, const Fetched& F) const {
    std::vector<uint8_t> skip(F.idx.size(), 0);
    const int64_t c_start = (int64_t)grid.start.at(g.iv.tid);
    for (size_t i = 0; i < F.idx.size(); i++) {
      const int64_t e_pos = F.set.pos(F.idx[i]);
      for (int64_t s1 = g.iv.start; s1 > c_start && e_pos < s1;) {   // grid intervals before this one, nearest first
        const int64_t s0 = std::max<int64_t>(c_start, s1 - (int64_t)a.sampling_interval_size);
        if (!bf || bf->overlaps(g.iv.tid, (uint64_t)s0, (uint64_t)s1)) { skip[i] = 1; break; }
        s1 = s0;
      }
    }
    return skip;
  }
  // the rest of an interval after its head (or all of it in full-data mode): sequential device rounds
  void finish_interval(const G& g, Fetched& head, size_t head_done, IntervalState* st) {
    const long limit = g.q.all ? -1 : (long)g.q.n;
    take(head, head_done, limit, g.iv.tid, true, st);
    if (!head.set.truncated(cap_of(g)) || (limit >= 0 && st->used >= (size_t)limit)) return;
    const size_t done = head.set.size();
    head.set = RecSet();
    // the head was not enough: the whole interval, records already seen skipped
    const Fetched whole = with_candidates(fetch(g.iv.tid, g.iv.start, g.iv.end, SIZE_MAX), &g);
    size_t from = 0; while (from < whole.idx.size() && whole.idx[from] < done) from++;
    take(whole, from, limit, g.iv.tid, true, st);
  }
  // intervals this rank samples, in order
  std::vector<const G*> my_intervals(const std::vector<G>& grouped) const {
    std::vector<const G*> mine;
    for (const G& g : grouped) {
      if (bf && !bf->overlaps(g.iv.tid, g.iv.start, g.iv.end)) continue;
      // owner of the interval: contiguous runs of the sampling grid by base pairs (as the pileup shards are dealt)
      if (sharded && grid.owner(g.iv, a.world) != a.rank) continue;
      mine.push_back(&g);
    }
    return mine;
  }
  struct Pending { const G* g; Fetched head; size_t n_first = 0; IntervalState st; };
  // the heads of the intervals gs[0, n), fetched concurrently (the head of the next one is fetched while the current one is looked at)
  std::vector<Pending> fetch_heads(const G* const* gs, size_t n) {
    std::vector<std::future<RecSet>> futs;
    // (resident: a scan of the digest, no fetch to overlap)
    for (size_t k = 0; k < n; k++) { const G* g = gs[k]; futs.push_back(std::async(resident_mode ? std::launch::deferred : std::launch::async,
        [this, g]() { return fetch(g->iv.tid, g->iv.start, g->iv.end, cap_of(*g)); })); }
    std::vector<Pending> pend(n);
    for (size_t k = 0; k < n; k++) {
      Pending& P = pend[k]; P.g = gs[k];
      auto t_f = std::chrono::steady_clock::now(); RecSet set = futs[k].get(); g_sample_times.fetch_ms += ms_since(t_f);
      P.head = with_candidates(std::move(set), P.g);
      P.n_first = P.g->q.all ? 0 : std::min(P.head.idx.size(), std::max<size_t>(256, 2 * P.g->q.n));
    }
    return pend;
  }
  // The count-based schedule needs only the head of every interval: the heads of consecutive intervals of one contig are decoded in ONE
  // device round; the sampler's first-N logic then runs over them in interval order.  An interval its head does not satisfy is finished
  // sequentially before the following ones are judged (their reads may already be taken by it), and the remaining heads are decoded again.
  void judge_heads(std::vector<Pending>& pend) {
    const uint32_t tid = pend[0].g->iv.tid;
    for (size_t k0 = 0; k0 < pend.size();) {
      Which recs; std::vector<size_t> at(pend.size() + 1, 0);
      for (size_t k = k0; k < pend.size(); k++) { at[k] = recs.size();
          for (size_t i = 0; i < pend[k].n_first; i++) recs.push_back({&pend[k].head.set, pend[k].head.idx[i]}); }
      at[pend.size()] = recs.size();
      std::vector<uint32_t> nv;
      auto t_d = std::chrono::steady_clock::now();
      device_round(recs, tid, true, &nv);
      g_sample_times.device_ms += ms_since(t_d); g_sample_times.rounds++; g_sample_times.reads += recs.size();
      auto t_h = std::chrono::steady_clock::now();
      std::vector<uint8_t> mask(recs.size(), 0);
      size_t unsatisfied = pend.size();
      for (size_t k = k0; k < pend.size(); k++) {
        Pending& P = pend[k]; const G& g = *P.g;
        verdict(P.head, 0, P.n_first, nv.data() + at[k], (long)g.q.n, &P.st, mask.data() + at[k]);
        const bool more = P.n_first < P.head.idx.size() || P.head.set.truncated(cap_of(g));
        if (P.st.used < g.q.n && more) { unsatisfied = k; break; }   // the judgement of the later heads waits for this interval
      }
      g_sample_times.decide_ms += ms_since(t_h);
      t_d = std::chrono::steady_clock::now();
      must(ctx, mkp_internal_sample_take(ctx, mask));
      g_sample_times.device_ms += ms_since(t_d);
      if (unsatisfied == pend.size()) break;
      Pending& P = pend[unsatisfied];
      finish_interval(*P.g, P.head, P.n_first, &P.st);
      k0 = unsatisfied + 1;
    }
  }
  // run_batch (reads_sampler/mod.rs:259-338) over the grouped intervals of one super batch: the heads of up to 8 consecutive intervals of one
  // contig (32 when they are scans of a resident shard's digest) go through fetch_heads / judge_heads together; an interval that takes all
  // of its reads goes alone
  void run_super_batch(const std::vector<G>& grouped) {
    std::map<uint32_t, size_t> batch_counts;
    const std::vector<const G*> mine = my_intervals(grouped);
    for (size_t mi = 0; mi < mine.size();) {
      const G& g0 = *mine[mi];
      size_t mj = mi + 1;
      // (resident: a head is a scan of the digest — more intervals per device round)
      if (!g0.q.all) while (mj < mine.size() && mj - mi < (resident_mode ? 32u : 8u) && !mine[mj]->q.all && mine[mj]->iv.tid == g0.iv.tid) mj++;
      std::vector<Pending> pend = fetch_heads(&mine[mi], mj - mi);
      if (g0.q.all) finish_interval(g0, pend[0].head, 0, &pend[0].st);
      else judge_heads(pend);
      for (auto& P : pend) batch_counts[P.g->iv.tid] += P.st.used;
      mi = mj;
    }
    for (auto& kv : batch_counts) sampled_so_far[kv.first] += kv.second;
  }

  // ---- the reads without a schedule
  // reads_sampler/mod.rs:89-125 (rank-sharded: rank 0 takes the unmapped reads)
  void unmapped_leg() {
    if (only_mapped || a.rank != 0) return;
    RecSet set; set.b.reset(new BamBatch()); bam.fetch_unmapped(set.b.get());
    const Fetched F = with_candidates(std::move(set));
    const long limit = a.have_frac ? -1 : (long)(a.num_reads > taken.size() ? a.num_reads - taken.size() : 0);
    // RecordSampler::new_from_options (record_sampler.rs:51-61): a fraction < 1 is a Bernoulli draw per record from StdRng — seeded by
    // --seed, else from entropy (no two runs of the reference agree: refused, --seed makes it a function of the input)
    const bool draws = a.have_frac && a.sampling_frac < 1.0;
    if (draws && !F.idx.empty() && !a.have_seed) throw Error(MKP_E_UNSUPPORTED,
        "unmapped-read sampling with --sampling-frac < 1 draws from an entropy-seeded rand::StdRng (record_sampler.rs:29-38): give --seed");
    SeededSampler rng(a.seed);
    IntervalState st;
    take(F, 0, limit, 0, false, &st, draws ? Draws{&rng, a.sampling_frac} : Draws());
  }
  // The sampler of a BAM WITHOUT an index (reads_sampler/mod.rs:129-158; `bam::IndexedReader::from_path(..).is_ok()` decides, so an index
  // ignored by `extract calls --ignore-index` still counts as one): no schedule — one pass over the file in file order, mapped and unmapped
  // records alike, under RecordSampler::new_from_options (record_sampler.rs:51-61): the first --num-reads records that yield values, or with
  // --sampling-frac one `gen_bool` per record the tag iterator yields (StdRng, --seed).  A region is an error there, as it is here.
  // Records go to the sampling kernels contig by contig (a round has one reference window and one BED mask); the sampler's state — reads
  // used, names seen — runs across the whole file: it is `take` with one IntervalState for the file (so its `seen` equals `taken` at every
  // step), no skip list, and the draws attached on every contig.
  void serial_pass(const RegionSpec* region) {
    if (region) throw Error(MKP_E_INVALID, "cannot use region without indexed BAM");
    const bool draws = a.have_frac && a.sampling_frac < 1.0;
    if (a.have_frac && a.sampling_frac > 1.0) throw Error(MKP_E_INVALID, "sample fraction must be <= 1");
    if (draws && !a.have_seed) throw Error(MKP_E_UNSUPPORTED,
        "--sampling-frac < 1 on a BAM without an index draws from an entropy-seeded rand::StdRng (record_sampler.rs:29-38): give --seed");
    // a draw is taken for every record whose tags parse and hold a position, whether or not a value survives the filters; the kernels report
    // surviving values only — the two coincide while nothing can remove a record's every position
    if (draws && (only_mapped || bf || !a.edge_filter.empty())) throw Error(MKP_E_UNSUPPORTED,
        "--sampling-frac < 1 on a BAM without an index together with --only-mapped / --include-bed / --edge-filter: which records consume a draw is not reproduced");
    SeededSampler rng(a.seed);
    const Draws d = draws ? Draws{&rng, a.sampling_frac} : Draws();
    const long limit = a.have_frac ? -1 : (long)a.num_reads;
    IntervalState st;
    auto more = [&]() { return limit < 0 || st.used < (size_t)limit; };   // (nothing is fetched once the limit is reached)
    for (size_t t = 0; t < bam.ref_names.size() && more(); t++) {
      RecSet set; set.b.reset(new BamBatch()); bam.fetch((uint32_t)t, 0, std::max<uint32_t>(bam.ref_lens[t], 1u), set.b.get());
      take(with_candidates(std::move(set)), 0, limit, (uint32_t)t, true, &st, d);
    }
    if (more()) { RecSet set; set.b.reset(new BamBatch()); bam.fetch_unmapped(set.b.get());
      take(with_candidates(std::move(set)), 0, limit, 0, false, &st, d); }
  }
};

// validate, build the quotas, then run the sampler's stages for every super batch
void sample_probabilities(mkp_ctx* ctx, const BamSource& bam, const Args& a, const RegionSpec* region, const BedFilter* bf,
    const ResidentOf& resident_of = ResidentOf()) {
  const bool only_mapped = !a.include_unmapped, sharded = a.world > 1;
  if (resident_of && (!only_mapped || sharded)) throw Error(MKP_E_INVALID, "internal: resident sampling needs mapped-only, single-rank sampling");
  ThresholdSampler sampler(ctx, bam, a, bf, resident_of);
  if (a.serial_sampler) { sampler.serial_pass(region); return; }
  if (sharded && !(a.have_frac && a.sampling_frac >= 1.0)) throw Error(MKP_E_UNSUPPORTED,
      "rank-sharded threshold sampling needs the full-data mode (-f 1.0): the count-based schedule carries quotas from interval to interval");
  const IdxStats st = idxstats(bam, region, bf);
  if ((only_mapped ? st.mapped : st.mapped + st.unmapped) == 0) throw Error(MKP_E_THRESHOLD, "zero reads found in bam index");
  if (a.have_frac && a.sampling_frac > 1.0) throw Error(MKP_E_INVALID, "sample fraction must be <= 1");
  const std::map<uint32_t, Quota> quota = a.have_frac ? quota_from_sample_frac(st, a.sampling_frac) : num_reads_quotas(st, a.num_reads, !only_mapped);
  const size_t batch_size = (size_t)floorf((float)a.threads * 1.5f);
  std::vector<Contig> contigs; for (auto& c : targets(bam, region)) if (quota.count(c.tid)) contigs.push_back(c);
  std::map<uint32_t, uint32_t> contig_size; for (auto& c : contigs) contig_size[c.tid] = c.length;
  sampler.grid = SamplingGrid(contigs);
  for (const std::vector<Iv>& all : sampling_super_batches(contigs, a.sampling_interval_size, batch_size))
    sampler.run_super_batch(group_super_batch(all, contig_size, quota, sampler.sampled_so_far));
  sampler.unmapped_leg();
}

// Full-data mode (`-f 1.0`, thresholds.rs:121-159) over shards that are resident in HBM.  sample_probabilities' schedule degenerates there
// to "every candidate read whose tags yield a value, once" — each sampling interval takes all of its reads, a read counts in the first
// interval it overlaps — so the shards are sampled directly, read by read in file order, without the interval machinery (and without its
// per-read std::set<std::string> lookups: 2.0 s of a 2.4 s run on the C4 scale model in round 4).  A read that lies in two shards of a
// contig belongs to the first one (`own_from`: the end of the previous shard's fetch), so the union over the shards — of one rank or of
// all ranks — is the single-rank sample; names seen before are skipped as the reference's Moniod keeps the first occurrence of a read id.
struct FullShard { uint32_t tid; int64_t own_from, ext_lo, ext_hi; std::function<const ShardHost*()> bind; };
void sample_resident_full(mkp_ctx* ctx, const BamSource& bam, const BedFilter* bf, std::vector<FullShard>& shards) {
  MaskSession mask_session(ctx);
  BedMasks bedmask_for{bf, bam, {}};
  std::unordered_set<NameKey, NameKeyHash> taken;
  for (auto& fs : shards) {
    auto t_f = std::chrono::steady_clock::now();
    const ShardHost* S = fs.bind();
    g_sample_times.fetch_ms += ms_since(t_f);
    if (!S || (int32_t)fs.tid != S->tid) throw Error(MKP_E_INVALID, "internal: resident sampling outside the ingested contigs");
    const std::vector<uint32_t> ids = resident_ids(*S, 0, S->hdr.size(), [&](const MkpReadHdr& h) {
      const int64_t pos = h.ref_start, end = std::max(h.ref_end, h.ref_start + 1);
      return pos >= fs.own_from && pos < fs.ext_hi && end > fs.ext_lo; });
    const uint8_t* mask = bedmask_for(fs.tid);
    for (size_t at = 0; at < ids.size();) {
      const size_t hi = std::min(ids.size(), at + ((size_t)1 << 18));
      std::vector<uint32_t> nv;
      auto t_d = std::chrono::steady_clock::now();
      must(ctx, mkp_internal_sample_resident(ctx, 0, bam.ref_lens[fs.tid], mask, ids.data() + at, (uint32_t)(hi - at), true, &nv));
      g_sample_times.device_ms += ms_since(t_d); g_sample_times.rounds++; g_sample_times.reads += hi - at;
      auto t_h = std::chrono::steady_clock::now();
      std::vector<uint8_t> take(hi - at, 0);
      for (size_t i = at; i < hi; i++) {
        if (nv[i - at] == 0) continue;   // a read that keeps no position is asked, not counted and not recorded
        if (taken.insert(resident_name_key(*S, ids[i])).second) take[i - at] = 1;
      }
      g_sample_times.decide_ms += ms_since(t_h);
      t_d = std::chrono::steady_clock::now();
      must(ctx, mkp_internal_sample_take(ctx, take));
      g_sample_times.device_ms += ms_since(t_d);
      at = hi;
    }
  }
}

// per-base pass thresholds from the context's resident sample: two-level histogram -> the two order statistics -> interpolation
void thresholds_from_sample(mkp_ctx* ctx, float q, float thr[4], uint8_t has[4], bool verbose, uint64_t* n_out = nullptr) {
  std::vector<uint64_t> h0(65536), h1(65536);
  for (uint32_t b = 0; b < 4; b++) {
    thr[b] = 0.f; has[b] = 0;
    must(ctx, mkp_histogram_get(ctx, b, 0, 0, h0.data()));
    uint32_t bins[2]; uint64_t rk[2], n = 0;
    int rc = mkp_histogram_locate(h0.data(), q, bins, rk, &n);
    if (n_out) n_out[b] = n;
    if (n == 0) continue;   // no calls on this base
    if (rc != MKP_OK) throw Error(MKP_E_THRESHOLD, "not enough datapoints, got " + std::to_string(n));
    float y[2];
    for (int k = 0; k < 2; k++) {
      if (k == 1 && bins[1] == bins[0] && rk[1] == rk[0]) { y[1] = y[0]; break; }
      if (k == 0 || bins[1] != bins[0]) must(ctx, mkp_histogram_get(ctx, b, 1, bins[k], h1.data()));
      rc = mkp_histogram_resolve(bins[k], h1.data(), rk[k], &y[k]);
        if (rc != MKP_OK) throw Error(MKP_E_THRESHOLD, "internal: histogram levels disagree");
    }
    float t; rc = mkp_percentile_from_histogram(n, q, y[0], y[1], &t);
      if (rc != MKP_OK) throw Error(MKP_E_THRESHOLD, "not enough datapoints, got " + std::to_string(n));
    thr[b] = t; has[b] = 1;
    if (verbose) fprintf(stderr, "[mkpileup] threshold %c %.9g (n=%llu)\n", "ACGT"[b], (double)t, (unsigned long long)n);
  }
}

void parse_base_thresholds(const std::vector<std::string>& raws, mkp_caller* k) {  // parse_per_base_thresholds (command_utils.rs:136-206)
  bool have_default = false;
  for (auto& raw : raws) {
    size_t c = raw.find(':');
    if (c != std::string::npos) {
      if (raw.find(':', c + 1) != std::string::npos || c == 0) throw Error(MKP_E_INVALID, "encountered illegal per-base threshold " + raw);
      int b = (int)std::string("ACGT").find(raw[0]); if (b < 0 || b > 3) throw Error(MKP_E_INVALID, "failed to parse base in " + raw);
      if (k->has_per_base[b]) throw Error(MKP_E_INVALID, "repeated threshold for base");
      k->has_per_base[b] = 1; k->per_base_threshold[b] = strtof(raw.c_str() + c + 1, nullptr);
    } else { if (have_default) throw Error(MKP_E_INVALID, "default threshold encountered more than once"); have_default = true;
        k->default_threshold = strtof(raw.c_str(), nullptr); }
  }
}

// The pileup driver's environment knobs, read from the environment when constructed.  The `MKP_NO_*` ones count when set to anything, the
// two ingest switches only when set to "1".
struct Knobs {
  static bool set(const char* k) { return getenv(k) != nullptr; }
  static bool one(const char* k) { const char* v = getenv(k); return v && !strcmp(v, "1"); }
  const bool trace = set("MKP_TRACE_PLAN");               // wall-clock marks of the subcommand's phases on stderr
  const bool device_inflate = one("MKP_DEVICE_INFLATE"), host_ingest = one("MKP_HOST_INGEST");   // as --device-inflate / --host-ingest
  const bool no_early_fetch = set("MKP_NO_EARLY_FETCH"), no_ahead = set("MKP_NO_AHEAD"), no_resident_sampling = set("MKP_NO_RESIDENT_SAMPLING"),
      no_bed_merge = set("MKP_NO_BED_MERGE");
  const char* const hbm_budget_mb = getenv("MKP_HBM_BUDGET_MB");   // overrides --hbm-budget-mb (0: 55 % of the device)
  // two shards in flight: a shard's own upload, block table and inflate overlap since the staged ingest, a second shard fills the gaps, and
  // more only crowd the short kernels of the threshold estimate beside them (C4 scale model, CLI: 1 worker 1.42 s, 2 1.22, 4 1.35, 8 1.34)
  const size_t ahead_workers = set("MKP_AHEAD_WORKERS") ? (size_t)std::max(1, atoi(getenv("MKP_AHEAD_WORKERS"))) : 2;
};

// --trace-plan marks: wall-clock time of the subcommand's phases on stderr
struct Marks {
  bool on; std::chrono::steady_clock::time_point t0;
  void operator()(const char* what) const { if (on) fprintf(stderr, "[mkpileup run] %-36s at %.1f ms\n", what, ms_since(t0)); }
};

// Option resolution (subcommand.rs:382-523): the flags checked in the reference's order (when several are wrong, the first check's message
// is the one the user sees), the caller config, the focus builder (motifs, BED, strand combining) and the writer's motif labels.  The
// reference FASTA loads on a thread of its own, joined where the grid walk needs it (load_fasta) or when this object dies.
struct Options {
  RegionSpec region, sregion; bool have_region = false, have_sregion = false;
  mkp_caller kc; std::vector<mkp_mod_threshold> per_mod;
  std::vector<Contig> records;   // the target records; under --include-bed the BED's (optimize_reference_records)
  BedFilter bed_store; const BedFilter* bf = nullptr;
  FocusBuilder fb; std::vector<std::string> labels;
  Fasta fasta; std::future<Fasta> fasta_load;
  Options(const Args& a, const BamSource& bam);
  ~Options() { if (fasta_load.valid()) fasta_load.wait(); }
  const RegionSpec* region_or_null() const { return have_region ? &region : nullptr; }
  void load_fasta(const Marks& mark) { if (fasta_load.valid()) { fasta = fasta_load.get(); fb.fasta = &fasta; mark("reference FASTA loaded"); } }
};

Options::Options(const Args& a, const BamSource& bam) {
  have_region = !a.region.empty(); have_sregion = !a.sample_region.empty();
  if (have_region) region = parse_region(a.region, bam);
  if (have_sregion) sregion = parse_region(a.sample_region, bam);
  memset(&kc, 0, sizeof(kc)); kc.max_depth = a.max_depth; kc.force_allow_implicit = a.force_allow;
  parse_edge_filter(a, &kc);
  per_mod = parse_mod_thresholds(a.mod_thresholds);
  records = targets(bam, region_or_null());
  if (!a.include_bed.empty()) { std::map<std::string, uint32_t> c2t; for (auto& r : records) c2t[r.name] = r.tid;
    bed_store = BedFilter::load(a.include_bed, c2t);
      bf = &bed_store; }
  if (idxstats(bam, region_or_null(), bf).mapped == 0) throw Error(MKP_E_INVALID,
      "did not find any mapped reads, perform alignment first or use modkit extract and/or modkit summary to inspect unaligned modBAMs");
  if (a.filter_percentile > 1.0f) throw Error(MKP_E_INVALID, "filter percentile must be <= 1.0");
  if (a.combine_strands && !(a.cpg || !a.motif_parts.empty())) throw Error(MKP_E_INVALID,
      "need to specify either --motif or --cpg to combine strands");
  // subcommand.rs:1247-1276: one motif, --cpg or --motif (a clap argument group: not both), palindromic; the reference FASTA is required
  if (a.hemi) {
    if (!a.cpg && a.motif_parts.empty()) throw Error(MKP_E_INVALID, "either --cpg or a --motif must be provided for pileup-hemi");
    if (a.cpg && !a.motif_parts.empty()) throw Error(MKP_E_INVALID, "the argument '--cpg' cannot be used with '--motif'");
    if (a.motif_parts.size() > 2) throw Error(MKP_E_INVALID, "motif arg should be length 2, eg. CG 0");
    if (a.ref_fasta.empty()) throw Error(MKP_E_INVALID, "the following required arguments were not provided: --ref <REFERENCE_FASTA>");
  }
  bool combine_strands = a.combine_strands;  // option resolution (subcommand.rs:484-523)
  if (a.preset == "traditional") { kc.numeric_mode = 2; kc.collapse_code = 'h'; combine_strands = true; }
  else if (!a.preset.empty()) throw Error(MKP_E_INVALID, "unknown preset " + a.preset);
  else if (a.combine_mods) kc.numeric_mode = 1;
  else if (!a.ignore.empty()) { uint32_t code; if (!parse_code(a.ignore, &code)) throw Error(MKP_E_INVALID, "failed to parse mod code " + a.ignore);
    kc.numeric_mode = 2;
      kc.collapse_code = code; }
  kc.combine_strands = combine_strands;
  if (a.hemi) combine_strands = true;
      // the interval feeder runs with combine_strands = true ("must be true for duplex", subcommand.rs:1383-1390); the caller's flag stays off
  fb.combine = combine_strands; fb.mask = a.mask; fb.bed = bf;
  if (!a.motif_parts.empty()) {  // RegexMotif::from_raw_parts (motif_bed.rs:152-195)
    if (!a.preset.empty()) throw Error(MKP_E_INVALID, "cannot use presets and motifs together");
    std::vector<std::string> parts = a.motif_parts;
    for (size_t i = 0; i + 1 < parts.size(); i += 2) for (size_t j = i + 2; j + 1 < parts.size(); j += 2) if (parts[i] == parts[j]
        && parts[i + 1] == parts[j + 1]) throw Error(MKP_E_INVALID,
        "cannot have the same motif more than once");
    if (a.cpg) { bool has = false; for (size_t i = 0; i + 1 < parts.size(); i += 2) if (parts[i] == "CG" && parts[i + 1] == "0") has = true;
        if (!has) { parts.push_back("CG"); parts.push_back("0"); } }
    for (size_t i = 0; i + 1 < parts.size(); i += 2) fb.motifs.push_back(Motif::parse(parts[i], strtoul(parts[i + 1].c_str(), nullptr, 10)));
  } else if (a.preset == "traditional" || a.cpg) fb.motifs.push_back(Motif::parse("CG", 0));
  for (auto& m : fb.motifs) labels.push_back(m.label());
  if (!fb.motifs.empty()) {
    if (a.ref_fasta.empty()) throw Error(MKP_E_INVALID, "reference fasta is required for using --motif or --cpg options");
    if (combine_strands) for (auto& m : fb.motifs) if (!m.palindrome) throw Error(MKP_E_INVALID,
        a.hemi ? "motif must be palindromic for pileup-hemi" : "cannot combine strands with a motif that is not a palindrome");
    // joined where the grid walk needs it: the device ingest of the first shard starts meanwhile
    fasta_load = std::async(std::launch::async, [&a]() { return Fasta::load(a.ref_fasta); });
  }
  if (bf) records = bed_contigs(*bf, records, a.interval_size);
}

// --device-inflate (or MKP_DEVICE_INFLATE=1): the shard windows' BGZF blocks are inflated on the GPU; the hook is removed and the inflater
// destroyed with this object
struct DeviceInflater {
  mkp_dev_inflater* d = nullptr; BamSource* src = nullptr;
  DeviceInflater(const Args& a, const Knobs& kn, BamSource& bam) {
    if (!((a.device_inflate || kn.device_inflate) && !a.plan_only && bam.indexed())) return;
    d = mkp_internal_inflater_create(a.device);
    if (!d) throw Error(MKP_E_DEVICE, "--device-inflate: cannot create a stream on the device");
    src = &bam; src->dev_inflate = mkp_internal_device_inflate; src->dev_inflate_user = d;
  }
  DeviceInflater(const DeviceInflater&) = delete;
  ~DeviceInflater() { if (src) { src->dev_inflate = nullptr; src->dev_inflate_user = nullptr; } mkp_internal_inflater_destroy(d); }
};

using Windows = std::vector<std::pair<uint32_t, uint32_t>>;
struct ShardInput { std::unique_ptr<BamBatch> batch; std::unique_ptr<DevShard> dev; };

// Reads the records of shards.  They come from the device ingest (mkp_ingest_host.cpp: compressed blocks up, inflate + record cut + tag
// tokeniser + packing in HBM, a digest back) whenever the BAM is indexed; --host-ingest / MKP_HOST_INGEST=1, --partition-tag (keys are read
// from aux fields on the host), --device-inflate and --plan-only keep the host reader + packer.  Owns the device inflater, so that it
// outlives every fetch made through this reader.
struct ShardReader {
  const BamSource& bam; mkp_ctx* ctx; DeviceInflater inflater; bool dev_ingest;
  ShardReader(const Args& a, const Knobs& kn, BamSource& src, mkp_ctx* c)
      : bam(src), ctx(c), inflater(a, kn, src),
        dev_ingest(src.indexed() && !a.plan_only && !a.host_ingest && a.partition_tags.empty() && !inflater.d && !kn.host_ingest) {
    if (dev_ingest && !ctx->ingest) { ctx->ingest = mkp_internal_ingest_create(ctx->device);
      if (!ctx->ingest) throw Error(MKP_E_DEVICE, "device ingest: cannot create streams on the device");
      }
  }
  // the records overlapping any of the windows (one window, or the BED spans of a merged shard), each +- the halo
  ShardInput fetch(uint32_t tid, const Windows& wins, mkp_dev_ingest* ing = nullptr) const {
    ShardInput in; FetchParts parts;
    for (auto& w : wins) { const int64_t lo = w.first > MKP_HALO ? (int64_t)w.first - MKP_HALO : 0, hi = (int64_t)w.second + MKP_HALO;
      if (!parts.empty() && lo <= parts.back().second) parts.back().second = std::max(parts.back().second, hi); else parts.push_back({lo, hi}); }
    // foreground: the upload feeds the GPU's longest job of the run
    if (dev_ingest) { in.dev = mkp_internal_ingest_run(ing ? ing : ctx->ingest, bam, tid, parts); return in; }
    HostPool::background() = true; in.batch.reset(new BamBatch()); bam.fetch_parts(tid, parts, in.batch.get()); return in;
  }
  // compressed bytes a set of fetch windows stands for (the index's 16 kb granularity: a short window costs at least its blocks)
  uint64_t win_bytes(uint32_t tid, const Windows& wins) const { uint64_t b = 0;
    for (auto& w : wins) b += bam.offset_at(tid, (uint64_t)w.second + 16384) - bam.offset_at(tid, w.first > 16384 ? w.first - 16384 : 0) + (1u << 16);
    return b; }
};

// Shards: pieces of the contig records cut at interval boundaries, bounded in positions (tally / focus buffers) and in BAM bytes (host
// memory: a shard's blocks are inflated and packed as a unit)
struct ShardSize {
  const BamSource& bam; uint64_t bp, bytes;
  ShardSize(const Args& a, const Knobs& kn, const BamSource& b, const std::vector<Contig>& records) : bam(b) {
    uint64_t total_bp = 0; for (auto& r : records) total_bp += r.length;
    bp = a.shard_bp ? a.shard_bp : (a.world > 1 ? std::max<uint64_t>(a.interval_size, std::min<uint64_t>(1ull << 27,
        (total_bp + a.world * 8 - 1) / (a.world * 8))) : (1ull << 27));
    // 2^27 positions per shard keeps the per-shard focus / slot buffers small
    // BAM bytes per shard: the device ingest's inflate pays a fixed latency per launch and HBM holds the window many times over — 1 GiB of
    // compressed blocks at a time; the host path keeps 256 MiB (its inflated window lives in host memory).  This predicate is not
    // ShardReader::dev_ingest: with MKP_DEVICE_INFLATE=1 and no --device-inflate it holds, and the 1 GiB shards go to the host packer.
    const bool dev_ingest_plan = !a.no_index && !a.plan_only && !a.host_ingest && a.partition_tags.empty() && !a.device_inflate
        && !kn.host_ingest;
    bytes = (a.shard_bytes_set || !dev_ingest_plan) ? a.shard_bytes : (1ull << 30);
  }
  // -> one past the shard's last interval
  size_t cut(const Contig& rec, const std::vector<Interval>& ivs, size_t i0, uint64_t* bp_out) const {
    size_t i1 = i0; uint64_t n = 0; const uint64_t o0 = bam.offset_at(rec.tid, ivs[i0].start);
    while (i1 < ivs.size() && (n == 0 || (n + (ivs[i1].end - ivs[i1].start) <= bp && (!bam.indexed() || bam.offset_at(rec.tid,
        ivs[i1].end) - o0 <= bytes)))) { n += ivs[i1].end - ivs[i1].start; i1++; }
    *bp_out = n; return i1;
  }
};

// The fetch windows of a shard made of `pieces` (ascending, disjoint) of contig `tid`: the pieces, or under --include-bed the BED spans
// inside them (rows exist at BED positions only; the records of optimize_reference_records run from one span to the next, most of what lies
// under them is never looked at).  Merged, ascending; empty when no BED position lies inside.
Windows shard_windows(const BedFilter* bf, uint32_t tid, const std::vector<Span>& pieces) {
  std::vector<Span> sp;
  if (!bf) sp = pieces;
  else if (!pieces.empty()) {   // the spans inside the hull, then what of them lies inside the pieces: one sweep
    size_t p = 0;
    for (auto& x : bf->spans_in(tid, pieces.front().s, pieces.back().e)) { while (p < pieces.size() && pieces[p].e <= x.s) p++;
      for (size_t q = p; q < pieces.size() && pieces[q].s < x.e; q++) {
        const uint64_t lo = std::max<uint64_t>(x.s, pieces[q].s), hi = std::min<uint64_t>(x.e, pieces[q].e);
        if (lo < hi) sp.push_back({lo, hi});
        } }
  }
  merge_spans(sp);
  Windows w; for (auto& x : sp) w.push_back({(uint32_t)x.s, (uint32_t)x.e});
  return w;
}

struct ShardPart { size_t rec; uint32_t s0, s1; };
struct ShardPlan { size_t rec; uint32_t s0, s1; uint64_t bp; std::vector<uint32_t> iv_starts; /* pileup-hemi: starts of the shard's intervals */
                   std::vector<ShardPart> parts; /* --include-bed: the BED-span records merged into this shard (empty: one window) */
                   int64_t own_from = INT64_MIN;
                     /* full-data sampling from the shards: reads starting before this position lie in the previous shard of the contig too, and are sampled there */ };

// the fetch windows of the shard [s0, s1) (made of `parts`, when merged)
Windows plan_windows(const BedFilter* bf, uint32_t tid, uint32_t s0, uint32_t s1, const std::vector<ShardPart>& parts = {}) {
  std::vector<Span> pieces; if (parts.empty()) pieces.push_back({s0, s1}); else for (auto& pt : parts) pieces.push_back({pt.s0, pt.s1});
  Windows w = shard_windows(bf, tid, pieces);
  if (w.empty()) w.push_back({s0, s0 + 1});   // (no BED position inside: nothing to fetch but an empty window)
  return w;
}

// Shards ingested AHEAD of the shard loop on worker threads, and kept packed in HBM (288 GB hold a 30x genome's packed reads): several target
// contigs (or the BED records of several contigs) each fitting one shard, or the plan's shards.  The threshold estimate may then sample from
// them (every contig's interval heads are scans of a digest, no second read of the file), and the pileup pass finds its shards already there.
// Several shards are in flight at once, each on an ingest object of its own (its streams, staging and scratch): one shard's inflate is a
// launch that fills a fraction of the chip for most of its time, and its host half (pread into staging) leaves the GPU idle — shards side by
// side fill both.  What they may hold is bounded by an HBM BUDGET (round 5; round 4 had an all-or-nothing 24 GiB gate on the compressed
// size): a shard is admitted — in plan order — while the estimated bytes of the admitted, not yet consumed shards fit the budget (one shard
// is always admitted), and the shard loop gives a shard's bytes back when it is through with it (release).  A run whose shards fit together
// keeps them all (and may sample its threshold estimate from them); a larger one streams.  The destructor stops and joins the workers, then
// destroys their ingest objects.
class AheadIngest {
 public:
  struct Shard { uint32_t tid = 0, s0 = 0, s1 = 0; Windows wins; ShardInput in; bool ready = false; std::exception_ptr err; uint64_t bytes = 0,
      est = 0; };
  std::vector<Shard> list;
  uint64_t budget = 0, est_total = 0;
  bool whole_contigs = false;   // the list holds whole contigs (from_contigs); the plan's shards may be pieces of them

  AheadIngest(const ShardReader& reader, mkp_ctx* ctx, uint64_t budget_mb, const Knobs& kn) : rd(reader), ctx(ctx), workers_wanted(kn.ahead_workers) {
    if (!rd.dev_ingest) return;
    const uint64_t mb = kn.hbm_budget_mb ? strtoull(kn.hbm_budget_mb, nullptr, 10) : budget_mb;
    if (mb) budget = mb << 20;
    else { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) != hipSuccess || !tot) tot = (size_t)64 << 30;
      budget = (uint64_t)((double)tot * 0.55); }
  }
  ~AheadIngest() {
    { std::lock_guard<std::mutex> g(mu); stop.store(true); }
    cv.notify_all();
    for (auto& t : workers) if (t.joinable()) t.join();
    for (auto* d : extra_ingest) mkp_internal_ingest_destroy(d);
  }
  bool empty() const { return list.empty(); }
  size_t size() const { return list.size(); }

  // packed arrays of a shard ~ 1.9 x its compressed blocks on ONT-like data (SEQ nibbles + CIGAR words + 5 bytes per call; names and
  // qualities are not kept), the inflated window of the ingest object in flight on top: 2.5 x; once the shard is resident, the slot
  // decoder's call and base planes (together four bits per stored base = as many bytes as the SEQ nibbles, ~1 x): 3.5 x; and the 16-bit CIGAR next
  // to the 32-bit one (half the CIGAR words' bytes, ~0.25 x): 3.75 x as the estimate
  static uint64_t est_of(uint64_t comp_bytes) { return comp_bytes * 15 / 4 + (64ull << 20); }

  // every target record as one shard, its records grouped by contig under --include-bed; nothing when one of them does not fit a shard
  // (a contig larger than a shard: the shards are cut on the grid and ingested ahead once the plan is known, from_plan)
  void from_contigs(const std::vector<Contig>& records, const BedFilter* bf, const ShardSize& size) {
    bool fits = true;
    for (size_t r0 = 0; r0 < records.size() && fits;) {
      size_t r1 = r0 + 1; if (bf) while (r1 < records.size() && records[r1].tid == records[r0].tid) r1++;
      Shard A; A.tid = records[r0].tid; A.s0 = records[r0].start; A.s1 = records[r1 - 1].end();
      std::vector<Span> pieces; for (size_t r = r0; r < r1; r++) pieces.push_back({records[r].start, records[r].end()});
      A.wins = shard_windows(bf, A.tid, pieces);
      A.bytes = bf ? rd.win_bytes(A.tid, A.wins) : rd.bam.offset_at(A.tid, A.s1) - rd.bam.offset_at(A.tid, A.s0);
      if ((uint64_t)A.s1 - A.s0 > size.bp || A.bytes > size.bytes || (bf && r1 - r0 > 65536) || records[r0].length == 0
          || A.wins.empty()) fits = false;
      list.push_back(std::move(A)); r0 = r1;
    }
    if (!fits) list.clear();
    whole_contigs = !list.empty();
    start();
  }
  // the plan's shards (several ranks, contigs larger than a shard, full-data sampling from the shards): same workers, same budget
  void from_plan(const std::vector<ShardPlan>& plan, const std::vector<Contig>& records, const BedFilter* bf) {
    if (!rd.dev_ingest || !list.empty() || plan.empty()) return;
    for (auto& sp : plan) { Shard A; A.tid = records[sp.rec].tid; A.s0 = sp.s0; A.s1 = sp.s1;
      A.wins = plan_windows(bf, A.tid, sp.s0, sp.s1, sp.parts);
      A.bytes = bf ? rd.win_bytes(A.tid, A.wins) : rd.bam.offset_at(A.tid, A.s1) - rd.bam.offset_at(A.tid, A.s0) + (1u << 16);
      list.push_back(std::move(A)); }
    start();
  }
  // shard k once its ingest is done (rethrows what the ingest threw)
  Shard& wait(size_t k) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return list[k].ready; });
    if (list[k].err) std::rethrow_exception(list[k].err); return list[k]; }
  // the shard loop is through with shard k
  void release(size_t k) { { std::lock_guard<std::mutex> g(mu); hbm_used -= std::min(hbm_used, list[k].est); } cv.notify_all(); }

 private:
  const ShardReader& rd; mkp_ctx* ctx; size_t workers_wanted;
  std::mutex mu; std::condition_variable cv; std::vector<std::thread> workers; std::atomic<bool> stop{false}; std::atomic<size_t> next{0};
  size_t admit_next = 0; uint64_t hbm_used = 0;   // (under mu)
  std::vector<mkp_dev_ingest*> extra_ingest;   // workers 1 ..; worker 0 ingests through the context's own

  void start() {
    if (list.empty() || !workers.empty()) return;
    est_total = 0; for (auto& A : list) { A.est = est_of(A.bytes); est_total += A.est; }
    size_t nw = std::min(workers_wanted, list.size());
    for (size_t w = 1; w < nw; w++) { mkp_dev_ingest* d = mkp_internal_ingest_create(ctx->device); if (!d) break; extra_ingest.push_back(d); }
    nw = extra_ingest.size() + 1;
    for (size_t w = 0; w < nw; w++) workers.emplace_back([this, w]() { work(w == 0 ? ctx->ingest : extra_ingest[w - 1]); });
  }
  void work(mkp_dev_ingest* ing) {
    for (;;) {
      const size_t k = next.fetch_add(1); if (k >= list.size()) break;
      { std::unique_lock<std::mutex> lk(mu);   // admission in plan order, under the budget
        cv.wait(lk, [&] { return stop.load() || (admit_next == k && (hbm_used == 0 || hbm_used + list[k].est <= budget)); });
        if (!stop.load()) { hbm_used += list[k].est; admit_next = k + 1; } }
      cv.notify_all();
      ShardInput in; std::exception_ptr err;
      if (stop.load()) err = std::make_exception_ptr(Error(MKP_E_INVALID, "internal: shard ingest cancelled"));
      else try { in = rd.fetch(list[k].tid, list[k].wins, ing); } catch (...) { err = std::current_exception(); stop.store(true); }
      { std::lock_guard<std::mutex> g(mu); list[k].in = std::move(in); list[k].err = err; list[k].ready = true; }
      cv.notify_all();
    }
  }
};

// The interval grid and focus bytes of every record — filled by the early walk (with one rank, on a thread of its own while the thresholds
// are estimated: both are all-cores work in short bursts, neither waits for the other's results) or where first needed — and the first
// shard's records, read and inflated early (behind the threshold estimate; background priority on the host pool, the estimate's own
// bursts go first).  The destructor joins the walk, then the early fetch the walk may have started.
struct Grid {
  std::vector<std::vector<uint8_t>> focus_of; std::vector<char> focus_done;
  std::vector<std::vector<Interval>> grid_of; std::vector<char> grid_done;
  double focus_ms = 0;
  std::future<ShardInput> early_fetch; uint32_t early_s0 = 0, early_s1 = 0; bool early_set = false;
  bool early_whole = false;   // the early fetch is the one target contig, begun before the grid was walked
  std::future<void> walk;
  explicit Grid(size_t n) : focus_of(n), focus_done(n, 0), grid_of(n), grid_done(n, 0) {}
  ~Grid() { if (walk.valid()) walk.wait(); if (early_fetch.valid()) early_fetch.wait(); }
  void join_walk() { if (walk.valid()) walk.get(); }   // rethrows what the walk threw
  void fetch_early(const ShardReader& rd, uint32_t tid, uint32_t s0, uint32_t s1) {
    early_s0 = s0; early_s1 = s1; early_set = true;
    early_fetch = std::async(std::launch::async, [&rd, tid, s0, s1]() { return rd.fetch(tid, {{s0, s1}}); });
  }
};

// The shard plan (ShardSize::cut); ranks take contiguous runs, balanced by the bytes the index puts under them (by length without an index).
// Built once, after the early walk is joined (the walker owns grid_of / focus_of until it is done).
struct Plan {
  std::vector<ShardPlan> shards;
  // what every rank's shards would hold in HBM if they were all ingested ahead (est_of of each shard's bytes under the index), computed by
  // every rank for every rank: the one thing a rank of a multi-GPU run may base a choice on that the other ranks must make the same way
  std::vector<uint64_t> est_by_rank;
  bool built = false;
};
void build_plan(Plan& p, const Args& a, const Knobs& kn, const BamSource& bam, Options& o, Grid& g, const ShardSize& size, bool ahead_listed,
    const Marks& mark) {
  if (p.built) return; p.built = true;
  g.join_walk();
  const std::vector<Contig>& records = o.records; const BedFilter* bf = o.bf; const bool hf = o.fb.has_focus();
  std::vector<ShardPlan>& plan = p.shards;
  p.est_by_rank.assign(std::max<uint32_t>(a.world, 1u), 0);
  {
    const uint64_t off_lo = records.empty() ? 0 : bam.offset_at(records.front().tid,
        records.front().start), off_hi = records.empty() ? 0 : bam.offset_at(records.back().tid, records.back().end());
    bool have_prev = false; uint32_t prev_tid = 0; int64_t prev_fetch_hi = 0;   // the shard before, over ALL ranks' shards: where its fetch ends
    for (size_t ri = 0; ri < records.size(); ri++) {
      const Contig& rec = records[ri];
      auto t_focus = std::chrono::steady_clock::now();
      // the grid; with one rank the focus bytes are filled in the same walk, otherwise only for the contigs this rank owns (below)
      std::vector<Interval> ivs;
      if (g.grid_done[ri]) ivs.swap(g.grid_of[ri]);
      else { ivs = o.fb.walk(rec, a.interval_size, (hf && a.world == 1) ? &g.focus_of[ri] : nullptr); if (hf && a.world == 1) g.focus_done[ri] = 1;
          g.focus_ms += ms_since(t_focus); }
      size_t i0 = 0;
      while (i0 < ivs.size()) {
        uint64_t bp = 0; const size_t i1 = size.cut(rec, ivs, i0, &bp); const uint64_t o0 = bam.offset_at(rec.tid, ivs[i0].start);
        const uint32_t s0 = ivs[i0].start, s1 = ivs[i1 - 1].end;
        const uint64_t mid = (o0 + bam.offset_at(rec.tid, s1)) / 2;
        const uint32_t owner = off_hi > off_lo ? (uint32_t)std::min<uint64_t>(a.world - 1,
            (mid > off_lo ? mid - off_lo : 0) * a.world / (off_hi - off_lo)) : 0;
        // the shard's intervals (pileup-hemi: per-interval NoCalls; always: the duplicate-name rule)
        std::vector<uint32_t> iv_starts; for (size_t k = i0; k < i1; k++) iv_starts.push_back(ivs[k].start);
        i0 = i1;
        const int64_t own_from = have_prev && prev_tid == rec.tid ? prev_fetch_hi : INT64_MIN;
        // (where the shard's last fetch window ends, before the halo)
        have_prev = true; prev_tid = rec.tid; prev_fetch_hi = (int64_t)plan_windows(bf, rec.tid, s0, s1).back().second + MKP_HALO;
        p.est_by_rank[owner] += AheadIngest::est_of(bam.indexed() ? bam.offset_at(rec.tid, s1) - o0 + (1u << 16) : 0);
        if (owner == a.rank) { plan.push_back({ri, s0, s1, bp, std::move(iv_starts)}); plan.back().own_from = own_from; }
      }
    }
  }
  // --include-bed: optimize_reference_records (position_filter.rs:103-210) turns every run of BED spans into a reference record of its own —
  // hundreds per contig for a sparse BED.  Rows only depend on the focus bytes (BED positions inside the records), not on how records are
  // grouped, so consecutive records of one contig share a shard: one hull window whose focus is zero between the records, fed by a
  // multi-window fetch of the records' spans only (what lies between them is neither read nor inflated).
  if (bf && plan.size() > 1 && !kn.no_bed_merge) {
    std::vector<ShardPlan> merged; uint64_t bytes = 0;
    for (auto& sp : plan) {
      const uint32_t tid = records[sp.rec].tid;
      const uint64_t sp_bytes = bam.indexed() ? bam.offset_at(tid, sp.s1) - bam.offset_at(tid, sp.s0) + (1u << 16) : 0;
      const bool join = !merged.empty() && records[merged.back().rec].tid == tid && sp.s0 >= merged.back().s1
          && (uint64_t)sp.s1 - merged.back().s0 <= size.bp
          && (bytes + sp_bytes <= size.bytes || ahead_listed /* its spans were sized when it was ingested ahead */) &&
                        merged.back().parts.size() < 65536;
      if (!join) { ShardPlan m = sp; m.parts.assign(1, {sp.rec, sp.s0, sp.s1}); merged.push_back(std::move(m)); bytes = sp_bytes; continue; }
      ShardPlan& m = merged.back(); m.s1 = sp.s1; m.bp += sp.bp; m.iv_starts.insert(m.iv_starts.end(), sp.iv_starts.begin(), sp.iv_starts.end());
        m.parts.push_back({sp.rec, sp.s0, sp.s1}); bytes += sp_bytes;
    }
    for (auto& m : merged) if (m.parts.size() == 1) m.parts.clear();
    plan.swap(merged);
  }
  mark("shard plan done");
}

// Where the run's time and work went: mkp_run_report and the --stats lines
struct Counters {
  std::chrono::steady_clock::time_point t_all;
  double load_ms = 0, thr_ms = 0, fetch_wait_early_ms = 0, grid_wait_ms = 0, callback_ms = 0, fetch_wait_ms = 0;
  double kernel_ms = 0, pack_ms = 0, h2d_ms = 0, d2h_ms = 0, dec_ms = 0, pil_ms = 0, row_ms = 0, write_ms = 0;
  uint64_t positions = 0, processed = 0, skipped = 0, n_shards = 0;
  uint64_t dev_rows = 0;   // rows the device produced (--region-stats-only: they never reach the writer, whose count is the report's otherwise)
  uint64_t n_wide = 0;   // shards that ran the wide-tally accumulate kernels (a column over 65 535 records deep)
  double ingest_ms[5] = {0, 0, 0, 0, 0}, ingest_kernel_ms = 0; uint64_t ingest_blocks = 0, ingest_records = 0, ingest_comp = 0, ingest_raw = 0;
  bool resident_used = false;   // the threshold sample came from shards in HBM

  void add_ingest(const DevShard& d) {
    ingest_ms[0] += d.ms_plan; ingest_ms[1] += d.ms_upload; ingest_ms[2] += d.ms_inflate; ingest_ms[3] += d.ms_pack; ingest_ms[4] += d.ms_digest;
    ingest_blocks += d.n_blocks; ingest_records += d.n_records; ingest_kernel_ms += d.ms_kernel; ingest_comp += d.comp_bytes; ingest_raw += d.raw_bytes;
  }
  void add_shard(mkp_ctx* ctx, uint64_t bp, const mkp_rows& rows) {
    n_shards++; n_wide += ctx->wide ? 1u : 0u;
    mkp_stats st; mkp_get_stats(ctx, &st); kernel_ms += st.kernel_ms; dec_ms += st.decode_kernel_ms; pil_ms += st.pileup_kernel_ms;
      row_ms += st.rows_kernel_ms;
        pack_ms += st.pack_ms; h2d_ms += st.h2d_ms; d2h_ms += st.d2h_ms; dev_rows += st.n_rows;
    positions += bp; processed += rows.processed_records; skipped += rows.skipped_records;
  }
  void report(mkp_run_report* rep, uint64_t n_rows, double focus_ms, const mkp_caller& kc) const {
    memset(rep, 0, sizeof(*rep));
    rep->load_ms = load_ms; rep->threshold_ms = thr_ms; rep->focus_ms = focus_ms; rep->pack_ms = pack_ms; rep->h2d_ms = h2d_ms;
      rep->kernel_ms = kernel_ms;
        rep->d2h_ms = d2h_ms; rep->write_ms = write_ms;
    rep->total_ms = ms_since(t_all); rep->n_rows = n_rows; rep->n_positions = positions; rep->n_shards = n_shards; rep->processed_records = processed;
        rep->skipped_records = skipped;
    for (int b = 0; b < 4; b++) { rep->threshold[b] = kc.per_base_threshold[b]; rep->has_threshold[b] = kc.has_per_base[b]; }
    rep->grid_wait_ms = grid_wait_ms; rep->callback_ms = callback_ms; rep->ingest_kernel_ms = ingest_kernel_ms; rep->ingest_upload_ms = ingest_ms[1];
      rep->ingest_table_ms = ingest_ms[0];
    rep->ingest_pack_ms = ingest_ms[3]; rep->ingest_comp_bytes = ingest_comp; rep->ingest_raw_bytes = ingest_raw; rep->ingest_blocks = ingest_blocks;
      rep->ingest_records = ingest_records;
  }
  void print_stats(const Args& a, const BamSource& bam, uint64_t n_rows, double focus_ms, bool dev_ingest, const AheadIngest& ahead) const {
    fprintf(stderr,
      "[mkpileup] rows=%llu positions=%llu processed~%llu skipped~%llu load_ms=%.1f threshold_ms=%.1f focus_ms=%.1f pack_ms=%.1f h2d_ms=%.1f kernel_ms=%.3f (decode %.3f pileup %.3f rows %.3f) d2h_ms=%.1f write_ms=%.1f total_ms=%.1f shards=%llu indexed=%d bam_bytes_read=%llu bam_bytes_inflated=%llu (on the device %llu) peak_rss_kb=%llu\n",
                       (unsigned long long)n_rows, (unsigned long long)positions, (unsigned long long)processed, (unsigned long long)skipped, load_ms,
                           thr_ms, focus_ms, pack_ms, h2d_ms, kernel_ms, dec_ms, pil_ms, row_ms, d2h_ms, write_ms, ms_since(t_all),
                       (unsigned long long)n_shards, bam.indexed() ? 1 : 0, (unsigned long long)bam.bytes_read.load(),
                           (unsigned long long)bam.bytes_inflated.load(), (unsigned long long)bam.bytes_inflated_device.load(),
                           (unsigned long long)peak_rss_kb());
    // every MKP_* variable that is set: they pick kernels and paths and would otherwise leave no trace in a measurement
    std::string ov; for (char** e = ::environ; e && *e; e++) if (!strncmp(*e, "MKP_", 4)) { ov += ' '; ov += *e; }
    fprintf(stderr,
        "[mkpileup] ingest=%s resident_sampling=%d ahead=%zu shards (estimated %.0f MB, HBM budget %.0f MB) rank=%u/%u env overrides:%s\n",
        dev_ingest ? "device" : "host", resident_used ? 1 : 0,
        ahead.size(), (double)ahead.est_total / 1048576.0, (double)ahead.budget / 1048576.0, a.rank, a.world, ov.empty() ? " none" : ov.c_str());
    if (n_wide) fprintf(stderr, "[mkpileup] wide tallies: %llu of %llu shards (columns deeper than 65535 records)\n", (unsigned long long)n_wide,
        (unsigned long long)n_shards);
    if (dev_ingest) fprintf(stderr,
      "[mkpileup] device ingest: %llu BGZF blocks, %llu records; block plan %.1f ms, upload %.1f, inflate + CRC + chains %.1f, parse + pack %.1f, digest %.1f (overlapped with the threshold estimate / the shard in hand)\n",
      (unsigned long long)ingest_blocks, (unsigned long long)ingest_records, ingest_ms[0], ingest_ms[1], ingest_ms[2], ingest_ms[3], ingest_ms[4]);
  }
};

// The first shard when the threshold estimate took it in hand: its records, or its device records already attached to the context
struct EarlyShard { ShardInput in; bool in_ready = false, attached = false; std::unique_ptr<DevShard> dev; };

// The one shard of the run is being ingested on the device and every read the schedule can ask for lies in it: the estimate waits for it and
// samples from HBM (the heads are scans of the shard's digest, a round is one launch over reads that are already packed) instead of fetching,
// inflating and packing interval heads on the host next to the ingest.  -> the shard attached to the context, or null
const ShardHost* attach_resident_shard(const Args& a, const BamSource& bam, Options& o, mkp_ctx* ctx, Grid& g, const ShardSize& size,
    const RegionSpec* sr, EarlyShard& early, Counters& c, const Marks& mark) {
  const std::vector<Contig>& records = o.records;
  { const IdxStats stx = idxstats(bam, sr, o.bf);
    for (auto& kv : stx.mapped_by_tid) if (kv.second && kv.first != (int64_t)records[0].tid) return nullptr; }
  mark("resident sampling: waiting for the grid");
  auto t_gw = std::chrono::steady_clock::now();
  if (g.walk.valid()) g.join_walk();
  else if (!g.grid_done[0]) { auto t_focus = std::chrono::steady_clock::now();
    g.grid_of[0] = o.fb.walk(records[0], a.interval_size, o.fb.has_focus() ? &g.focus_of[0] : nullptr); g.grid_done[0] = 1;
    if (o.fb.has_focus()) g.focus_done[0] = 1; g.focus_ms += ms_since(t_focus); }
  c.grid_wait_ms += ms_since(t_gw);
  const std::vector<Interval>& ivs = g.grid_of[0]; uint64_t bp = 0;
  if (ivs.empty() || size.cut(records[0], ivs, 0, &bp) != ivs.size() || ivs.front().start != g.early_s0 || ivs.back().end != g.early_s1)
    return nullptr;
  // the shard is begun and everything of its plan that needs the window alone (slot bitmap, slot positions, their uploads) is made now,
  // while the ingest is still running
  mkp_shard sh; memset(&sh, 0, sizeof(sh)); sh.tid = (int32_t)records[0].tid; sh.start = g.early_s0; sh.end = g.early_s1;
  if (o.fb.has_focus()) { sh.focus = g.focus_of[0].data() + (g.early_s0 - records[0].start); sh.combos = o.fb.combos.data();
    sh.n_combos = (uint32_t)o.fb.combos.size(); }
  must(ctx, mkp_shard_begin(ctx, &sh));
  { std::vector<uint32_t> st; st.reserve(ivs.size()); for (auto& iv : ivs) st.push_back(iv.start);
    must(ctx, mkp_shard_set_intervals(ctx, st.data(), (uint32_t)st.size())); }
  if (o.fb.has_focus() && !a.hemi) must(ctx, mkp_internal_shard_preplan(ctx));
  auto t_w = std::chrono::steady_clock::now();
  mark("resident sampling: waiting for the ingest");
  early.in = g.early_fetch.get(); early.in_ready = true;
  c.fetch_wait_early_ms = ms_since(t_w);
  mark("resident sampling: ingest in hand");
  if (!early.in.dev) return nullptr;
  early.dev = std::move(early.in.dev); early.in_ready = false;
  must(ctx, mkp_internal_shard_attach(ctx, early.dev.get())); mkp_internal_ingest_recycle(ctx->ingest, early.dev.get());
  early.attached = true;
  mark("first shard attached (resident sampling)");
  return &ctx->shard;
}

// The threshold estimate (subcommand.rs:615-638) -> kc's per-base thresholds.  The sample comes from the shard attached for it, from the
// shards ingested ahead (full-data mode: whatever their cut; count-based: when they are the whole contigs), or through the host sampler —
// unless mkp_pileup_run_cb's callback supplies the thresholds.
void estimate_thresholds(const Args& a, const Knobs& kn, const BamSource& bam, Options& o, mkp_ctx* ctx, Grid& g, AheadIngest& ahead,
    const Plan& plan, const ShardSize& size, bool dev_ingest, bool resident_ok, EarlyShard& early, Counters& c, const Marks& mark) {
  const bool full_mode = a.have_frac && a.sampling_frac >= 1.0;
  auto t0 = std::chrono::steady_clock::now();
  must(ctx, mkp_set_caller(ctx, &o.kc));  // collapse + edge filter apply to the sampled probabilities too
  const RegionSpec* sr = o.have_sregion ? &o.sregion : o.region_or_null();
  // a rank of a multi-GPU run that was not handed thresholds (--filter-threshold from the all-reduced histograms, see
  // modkit_amd.distributed) estimates them alone over the whole file: correct, but every rank repeats the work
  Args as = a; as.world = 1; as.rank = 0;
  must(ctx, mkp_histogram_begin(ctx));
  g_sample_times = SampleTimes();
  // mkp_pileup_run_cb: in the count-based modes the caller supplies the thresholds (one rank estimates, all ranks receive: the schedule
  // carries quotas from interval to interval and does not shard) — nothing is sampled here, and this rank's shards are being ingested
  // meanwhile; in the full-data mode this rank samples its own shards and the caller reduces the histograms over the ranks
  const bool cb_supplies = a.thr_cb && !full_mode;
  if (!cb_supplies) {
    const ShardHost* resident = g.early_whole && resident_ok ? attach_resident_shard(a, bam, o, ctx, g, size, sr, early, c, mark) : nullptr;
    ResidentOf resident_of;
    DevShard* bound = nullptr;   // multi-shard resident sampling: the shard currently swapped into the context
    struct Unbind { mkp_ctx* c; DevShard** b; ~Unbind() { if (*b) { (void)mkp_internal_sample_bind(c, *b); *b = nullptr; } } } unbind{ctx, &bound};
    auto bind_ahead = [&](size_t k) -> const ShardHost* {
      auto t_w = std::chrono::steady_clock::now();
      AheadIngest::Shard& A = ahead.wait(k);
      c.fetch_wait_early_ms += ms_since(t_w);
      if (!A.in.dev) throw Error(MKP_E_INVALID, "internal: shard ingested ahead without device records");
      if (bound != A.in.dev.get()) { if (bound) must(ctx, mkp_internal_sample_bind(ctx, bound)); bound = nullptr;
        must(ctx, mkp_internal_sample_bind(ctx, A.in.dev.get())); bound = A.in.dev.get(); }
      return &ctx->shard;
    };
    // every shard stays in HBM until the loop takes it: the sample can come from them
    const bool ahead_fits = !ahead.empty() && ahead.est_total <= ahead.budget;
    // the extent the sampler covers on a contig: the region, or all of it
    auto ext_of = [&](uint32_t tid, int64_t* lo, int64_t* hi) { if (o.have_region) { *lo = o.region.start; *hi = o.region.end; } else { *lo = 0;
        *hi = bam.ref_lens[tid]; } };
    // Several ranks in the full-data mode (mkp_pileup_run_cb): the ranks' samples are summed by the caller, so every rank must cut the reads the
    // same way — by shard ownership (own_from) when the shards are the source, by sampling intervals when the host reader is.  The two cuts do
    // not coincide, so the choice is one every rank arrives at alike without talking: the shards are the source iff EVERY rank's shards fit
    // its budget (est_by_rank: the same arithmetic on the same index on every rank; the budget and MKP_NO_AHEAD must be the ranks' common
    // setting, like the flags).  A rank without shards then contributes an empty sample (it used to sample its bp-share of the
    // sampling intervals, reads the other ranks' shards had already counted).
    bool all_ranks_resident = dev_ingest && plan.built && !kn.no_ahead && !g.early_whole;
    for (uint64_t e : plan.est_by_rank) if (e > ahead.budget) all_ranks_resident = false;
    const bool shards_are_the_sample = a.world > 1 ? (a.thr_cb && all_ranks_resident) : ahead_fits;
    if (full_mode && resident_ok && (resident || shards_are_the_sample)) {
      // full-data mode: the shards themselves are the sample's source, whatever their cut — with several ranks (mkp_pileup_run_cb) each
      // rank its own, the caller sums the histograms
      std::vector<FullShard> fs;
      if (resident) { FullShard f; f.tid = o.records[0].tid; f.own_from = INT64_MIN; ext_of(f.tid, &f.ext_lo, &f.ext_hi); f.bind = [&]() {
          return resident; }; fs.push_back(std::move(f)); }
      else for (size_t k = 0; k < ahead.size(); k++) { FullShard f; f.tid = ahead.list[k].tid;
        f.own_from = ahead.whole_contigs ? INT64_MIN : plan.shards[k].own_from; ext_of(f.tid, &f.ext_lo, &f.ext_hi);
          f.bind = [&, k]() { return bind_ahead(k); }; fs.push_back(std::move(f)); }
      sample_resident_full(ctx, bam, o.bf, fs);
      c.resident_used = true;
      if (a.stats) fprintf(stderr, "[mkpileup] full-data threshold sample taken from %zu resident shard(s)%s\n", fs.size(),
          a.world > 1 ? " of this rank" : "");
    } else {
    if (resident) resident_of = [&](uint32_t) { return resident; };
    else if (ahead_fits && ahead.whole_contigs && resident_ok && a.world == 1) {
      // every contig the schedule can visit must be among the shards ingested ahead
      std::map<uint32_t, size_t> by_tid; for (size_t k = 0; k < ahead.size(); k++) by_tid[ahead.list[k].tid] = k;
      bool covered = true; { const IdxStats stx = idxstats(bam, sr, o.bf);
        for (auto& kv : stx.mapped_by_tid) if (kv.second && !by_tid.count((uint32_t)kv.first)) covered = false;
        }
      // (a region run: the one record is the region; a BED run: a contig's shard holds the records reaching its BED spans, which are the only ones
      // that can yield a value)
      if (covered) resident_of = [&, by_tid](uint32_t tid) -> const ShardHost* {
        auto it = by_tid.find(tid); if (it == by_tid.end()) throw Error(MKP_E_INVALID, "internal: resident sampling outside the ingested contigs");
        return bind_ahead(it->second);
      };
    }
    // (a rank of mkp_pileup_run_cb's full-data mode whose shards are not resident — an unindexed BAM, a budget too small — samples its own
    // sampling intervals through the host reader, as round 4 did)
    sample_probabilities(ctx, bam, (a.thr_cb && full_mode) ? a : as, sr, o.bf, resident_of);
    if (resident_of) c.resident_used = true;
    if (a.stats && resident_of && !resident) fprintf(stderr, "[mkpileup] threshold estimate sampled from %zu shards ingested ahead (resident)\n",
        ahead.size());
    }
    if (bound) { must(ctx, mkp_internal_sample_bind(ctx, bound)); bound = nullptr; }
    mark("schedule walked, sample in HBM");
    if (a.stats) fprintf(stderr,
        "[mkpileup] threshold sampling: head fetch wait %.1f ms, device rounds %llu (%llu reads) %.1f ms, first-N logic %.1f ms\n",
        g_sample_times.fetch_ms, (unsigned long long)g_sample_times.rounds, (unsigned long long)g_sample_times.reads, g_sample_times.device_ms,
        g_sample_times.decide_ms);
  }
  { float thr[4] = {0, 0, 0, 0}; uint8_t has[4] = {0, 0, 0, 0};
    if (a.thr_cb) { auto t_cb = std::chrono::steady_clock::now(); const int rc = a.thr_cb(a.thr_cb_user, ctx, cb_supplies ? 0 : 1, thr, has);
      c.callback_ms = ms_since(t_cb);
      if (rc != MKP_OK) throw Error(rc, "the threshold callback failed"); mark("thresholds from the callback"); }
    else thresholds_from_sample(ctx, a.filter_percentile, thr, has, a.stats);
    for (int b = 0; b < 4; b++) if (has[b]) { o.kc.has_per_base[b] = 1; o.kc.per_base_threshold[b] = thr[b]; } }
  c.thr_ms = ms_since(t0) - c.fetch_wait_early_ms - c.grid_wait_ms - c.callback_ms;
}

// Where the rows go: one bedMethyl file (plain or BGZF + index), one per --partition-tag key in a directory, or --bedgraph files
class Outputs {
 public:
  // the checks throw in the order of the flags' resolution (subcommand.rs:328-363 for --bedgraph)
  Outputs(const Args& a, mkp_ctx* ctx, const std::vector<std::string>& labels) : a(a), partitioned(!a.partition_tags.empty()) {
    wr.mixed = a.mixed_delim; wr.labels = labels;
    if (a.rows_stay()) return;   // no rows reach the host: nothing is opened (every shard hands write() zero rows)
    if (a.bedgraph) {   // (no header, no mixed delimiters; the path is a directory)
      if (a.with_header || a.mixed_delim || a.bgzf || a.hemi || a.plan_only) throw Error(MKP_E_INVALID,
          "--bedgraph cannot be combined with --with-header, --mixed-delim, --bgzf or --plan-only");
      if (a.out_bed.empty() || a.out_bed == "-" || a.out_bed == "stdout") throw Error(MKP_E_INVALID, "--bedgraph needs an output directory");
      if (partitioned) set_partition_tags(ctx);
      make_dir();
      bg.dir = a.out_bed; bg.prefix = a.prefix; bg.groupings = partitioned; bg.labels = wr.labels;
    } else if (partitioned) {   // a directory with one bedMethyl per key, `[<prefix>_]<key>.bed` (PartitioningBedMethylWriter, writers.rs:1005-1082)
      if (a.with_header) throw Error(MKP_E_INVALID, "--with-header cannot be combined with --partition-tag");
      if (a.plan_only) throw Error(MKP_E_INVALID, "--plan-only has no partitioned form");
      set_partition_tags(ctx);
      make_dir();
    } else {
      wr.f = (a.out_bed == "-" || a.out_bed == "stdout" || (a.hemi && a.out_bed.empty())) ? stdout : fopen(a.out_bed.c_str(), "w+");
      if (!wr.f) throw Error(MKP_E_IO, "failed to make output file " + a.out_bed);
      if (a.bgzf) {
        if (wr.f == stdout || a.with_header || a.plan_only) throw Error(MKP_E_INVALID,
            "--bgzf writes a file and its index: it needs an output path and goes without --with-header");
        wr.bz.reset(new BgzfTabixSink()); wr.bz->f = wr.f; wr.bz->index_path = a.out_bed + ".tbi";
      }
    }
    if (a.bgzf && partitioned) throw Error(MKP_E_INVALID, "--bgzf has no partitioned form");
    if (a.with_header) fputs("chrom\tchromStart\tchromEnd\tname\tscore\tstrand\tthickStart\tthickEnd\tcolor\tvalid_coverage\tpercent_modified\tcount_modified\tcount_canonical\tcount_other_mod\tcount_delete\tcount_fail\tcount_diff\tcount_nocall\n",
        wr.f);
  }
  FILE* file() const { return wr.f; }   // (--plan-only: the plan TSV)
  uint64_t rows() const { return wr.n; }
  void write(const std::string& chrom, const mkp_rows& rows) {
    if (a.bedgraph) { bg.write(chrom, rows); wr.n += rows.n_rows; }
    else if (!partitioned) wr.write(chrom, rows);
    else for (uint64_t i0r = 0; i0r < rows.n_rows;) {   // rows come grouped by key: one slice per key
      uint64_t i1r = i0r; while (i1r < rows.n_rows && rows.partition_key[i1r] == rows.partition_key[i0r]) i1r++;
      mkp_rows v = rows; v.n_rows = i1r - i0r; v.pos += i0r; v.strand += i0r; v.code_repr += i0r; v.motif_idx += i0r; v.n_valid += i0r;
        v.n_mod += i0r;
          v.n_canonical += i0r; v.n_other += i0r;
      v.n_delete += i0r; v.n_fail += i0r; v.n_diff += i0r; v.n_nocall += i0r; v.partition_key += i0r;
      const uint32_t k = rows.partition_key[i0r];
      RowWriter& kw = writer_for(k < rows.n_partition_keys ? rows.partition_key_names[k] : "not_found"); kw.write(chrom, v); wr.n += v.n_rows;
      i0r = i1r;
    }
  }
  void write_hemi(const std::string& chrom, const mkp_hemi_rows& rows) { wr.write_hemi(chrom, rows); }
  void finish() {
    bg.finish(); wr.finish(); for (auto& kv : key_writers) { kv.second->finish(); fclose(kv.second->f); }
  }
  void close() { if (wr.f && wr.f != stdout) fclose(wr.f); }

 private:
  const Args& a; const bool partitioned;
  RowWriter wr; BedGraphOut bg; std::map<std::string, std::unique_ptr<RowWriter>> key_writers;
  void set_partition_tags(mkp_ctx* ctx) { std::vector<const char*> tp; for (auto& t : a.partition_tags) tp.push_back(t.c_str());
    must(ctx, mkp_set_partition_tags(ctx, tp.data(), (uint32_t)tp.size())); }
  void make_dir() { if (mkdir(a.out_bed.c_str(), 0777) != 0 && errno != EEXIST) throw Error(MKP_E_IO, "failed to make output directory " + a.out_bed); }
  RowWriter& writer_for(const std::string& key) {
    auto it = key_writers.find(key);
    if (it == key_writers.end()) {
      std::unique_ptr<RowWriter> w(new RowWriter()); w->mixed = a.mixed_delim; w->labels = wr.labels;
      const std::string path = a.out_bed + "/" + (a.prefix.empty() ? key : a.prefix + "_" + key) + ".bed";
      w->f = fopen(path.c_str(), "w+"); if (!w->f) throw Error(MKP_E_IO, "failed to make output file " + path);
      it = key_writers.emplace(key, std::move(w)).first;
    }
    return *it->second;
  }
};

// --plan-only: a host-only dry run of one shard — its plan line, plus the packer over its records (no device)
void plan_only_shard(const Args& a, const Contig& rec, uint32_t s0, uint32_t s1, const std::vector<mkp_record>& recs, FILE* out, Counters& c) {
  static std::vector<ShardHost> kept_pieces;   // the all-cores pack's per-thread buffers persist across shards, as they do in a context
  Packer pk; pk.pieces.swap(kept_pieces); ShardHost S; S.tid = (int32_t)rec.tid; S.win_start = (int32_t)s0; S.win_end = (int32_t)s1;
  const int32_t tid = (int32_t)rec.tid; auto t_pk = std::chrono::steady_clock::now();
  // --plan-pack-min N: records from which the packer runs on all cores (0 = always; default as in mkp_shard_add_records)
  pack_records(pk, S, recs.data(), (uint32_t)recs.size(), [tid](const mkp_record& r) { return r.tid == tid && Packer::keep(r);
    }, a.plan_pack_min);
  c.pack_ms += ms_since(t_pk); kept_pieces.swap(pk.pieces);
  // digest of everything the packer hands to the device: a parallel pack must equal the sequential one byte for byte
  uint64_t dg = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; for (size_t i = 0; i < n; i++) { dg ^= b[i];
      dg *= 1099511628211ull; } };
  mix(S.hdr.data(), S.hdr.size() * sizeof(MkpReadHdr)); mix(S.cigar.data(), S.cigar.size() * 4); mix(S.cigar16.data(), S.cigar16.size() * 2);
    mix(S.chunk_pfx.data(), S.chunk_pfx.size() * 4);
      mix(S.seq.data(), S.seq.size());
  mix(S.tagref.data(), S.tagref.size() * sizeof(MkpTagRef)); mix(S.ranks.data(), S.ranks.size() * 4); mix(S.ml.data(), S.ml.size());
      mix(S.name_hash.data(), S.name_hash.size() * 8);
  for (auto& k : pk.layout_keys) mix(k.data(), k.size());
  fprintf(out, "%s\t%u\t%u\t%zu\t%llu\t%016llx\n", rec.name.c_str(), s0, s1, S.hdr.size(), (unsigned long long)S.n_calls,
      (unsigned long long)dg);
}

// The shard loop: every shard of the plan fetched (or taken from those ingested ahead / the one attached for the estimate), packed, run on
// the device and written.  Double buffering: the next shard's blocks are read and inflated while this one is packed, run and written.
void run_shards(const Args& a, Options& o, mkp_ctx* ctx, const ShardReader& reader, Grid& g, AheadIngest& ahead, const Plan& p,
    EarlyShard& early, Outputs& out, Counters& c, const Marks& mark) {
  const std::vector<ShardPlan>& plan = p.shards; const std::vector<Contig>& records = o.records; const bool hf = o.fb.has_focus();
  auto fetch_shard = [&](const ShardPlan& sp) { const uint32_t tid = records[sp.rec].tid;
    return reader.fetch(tid, plan_windows(o.bf, tid, sp.s0, sp.s1, sp.parts)); };
  // shards that were ingested ahead: same contig, same hull, same windows
  std::vector<long> plan_ahead(plan.size(), -1);
  for (size_t pi = 0; pi < plan.size(); pi++) for (size_t k = 0; k < ahead.size(); k++) {
    const AheadIngest::Shard& A = ahead.list[k]; const uint32_t tid = records[plan[pi].rec].tid;
    if (A.tid == tid && A.s0 == plan[pi].s0 && A.s1 == plan[pi].s1 && A.wins == plan_windows(o.bf, tid, plan[pi].s0, plan[pi].s1, plan[pi].parts)) {
      plan_ahead[pi] = (long)k; break; } }
  std::future<ShardInput> next_batch;
  const bool early_match = g.early_set && !plan.empty() && plan[0].rec == 0 && plan[0].s0 == g.early_s0 && plan[0].s1 == g.early_s1;
  if (early.attached && !(early_match && plan.size() == 1)) throw Error(MKP_E_INVALID,
      "internal: the shard attached for resident sampling is not the plan's");
  // (what the estimate waited for shards ingested ahead is load time too)
  if (early.attached || !ahead.empty()) { c.fetch_wait_ms += c.fetch_wait_early_ms; }
  else if (early_match && early.in_ready) { c.fetch_wait_ms += c.fetch_wait_early_ms; next_batch = std::async(std::launch::deferred, [&]() {
      return std::move(early.in); }); }
  else if (early_match && g.early_fetch.valid()) next_batch = std::move(g.early_fetch);
  else { if (g.early_fetch.valid()) g.early_fetch.wait();
    if (!plan.empty() && plan_ahead[0] < 0) next_batch = std::async(std::launch::async, fetch_shard, plan[0]);
    }
  for (size_t pi = 0; pi < plan.size(); pi++) {
    const ShardPlan& sp = plan[pi]; const Contig& rec = records[sp.rec]; const uint32_t s0 = sp.s0, s1 = sp.s1;
    std::unique_ptr<BamBatch> batch; std::unique_ptr<DevShard> dev;
    const bool attached_already = early.attached && pi == 0;
    // the shard's bytes go back to the budget when this iteration is over
    struct Release { AheadIngest& ahead; long k; ~Release() { if (k >= 0) ahead.release((size_t)k); } } release_shard{ahead, plan_ahead[pi]};
    if (attached_already) dev = std::move(early.dev);
    else if (plan_ahead[pi] >= 0) { auto t_f = std::chrono::steady_clock::now(); AheadIngest::Shard& A = ahead.wait((size_t)plan_ahead[pi]);
      batch = std::move(A.in.batch); dev = std::move(A.in.dev); c.fetch_wait_ms += ms_since(t_f); }
    else { auto t_f = std::chrono::steady_clock::now(); ShardInput in = next_batch.get(); batch = std::move(in.batch); dev = std::move(in.dev);
      c.fetch_wait_ms += ms_since(t_f); }
    if (dev) c.add_ingest(*dev);
    if (pi + 1 < plan.size() && plan_ahead[pi + 1] < 0) next_batch = std::async(std::launch::async, fetch_shard, plan[pi + 1]);
    std::vector<uint8_t> merged_focus;   // a merged shard: its records' focus bytes at their places in the hull, zero in between
    if (hf) for (size_t k = 0; k < std::max<size_t>(sp.parts.size(), 1); k++) { const size_t ri = sp.parts.empty() ? sp.rec : sp.parts[k].rec;
      if (!g.focus_done[ri]) { auto t_focus = std::chrono::steady_clock::now(); o.fb.walk(records[ri], a.interval_size, &g.focus_of[ri]);
        g.focus_done[ri] = 1; g.focus_ms += ms_since(t_focus); } }
    if (sp.rec > 0 && (pi == 0 || plan[pi - 1].rec != sp.rec)) for (size_t r2 = 0; r2 < sp.rec; r2++) { std::vector<uint8_t>().swap(g.focus_of[r2]);
        }   // earlier contigs are done
    if (hf && !sp.parts.empty()) { merged_focus.assign((size_t)(s1 - s0), 0);
      for (auto& pt : sp.parts) memcpy(merged_focus.data() + (pt.s0 - s0), g.focus_of[pt.rec].data() + (pt.s0 - records[pt.rec].start),
          (size_t)(pt.s1 - pt.s0));
        }
    const std::vector<uint8_t>& focus = g.focus_of[sp.rec];
    std::vector<mkp_record> recs; if (batch) { recs.reserve(batch->recs.size()); for (auto& e : batch->recs) recs.push_back(batch->view(e)); }
    if (a.plan_only) { plan_only_shard(a, rec, s0, s1, recs, out.file(), c); c.positions += sp.bp; continue; }
    mkp_shard sh; memset(&sh, 0, sizeof(sh)); sh.tid = (int32_t)rec.tid; sh.start = s0; sh.end = s1;
    if (hf) { sh.focus = sp.parts.empty() ? focus.data() + (s0 - rec.start) : merged_focus.data(); sh.combos = o.fb.combos.data();
      sh.n_combos = (uint32_t)o.fb.combos.size(); }
    mark("shard blocks in hand");
    if (attached_already) dev.reset();   // begun and attached before the threshold estimate, which sampled from it
    else {
      must(ctx, mkp_shard_begin(ctx, &sh));
      must(ctx, mkp_shard_set_intervals(ctx, sp.iv_starts.data(), (uint32_t)sp.iv_starts.size()));
      if (dev) { must(ctx, mkp_internal_shard_attach(ctx, dev.get())); mkp_internal_ingest_recycle(ctx->ingest, dev.get()); dev.reset(); }
      else must(ctx, mkp_shard_add_records(ctx, recs.data(), (uint32_t)recs.size()));
    }
    mark("shard packed");
    batch.reset();   // packed: the inflated blocks are no longer needed (their mappings are parked for the next fetch, ByteBuf::spares)
    mkp_rows rows; memset(&rows, 0, sizeof(rows));
    if (a.hemi) {
      int hoff = 0; o.fb.motifs[0].neg_delta(&hoff);
      mkp_hemi_rows hrows; must(ctx, mkp_hemi_shard_run(ctx, hoff, sp.iv_starts.data(), (uint32_t)sp.iv_starts.size(), &hrows));
      if (a.rerun) must(ctx, mkp_shard_rerun(ctx, a.rerun, nullptr));
      auto t_w = std::chrono::steady_clock::now();
      out.write_hemi(rec.name, hrows);
      c.write_ms += ms_since(t_w);
      rows.processed_records = hrows.processed_records; rows.skipped_records = hrows.skipped_records;
    } else {
      must(ctx, mkp_shard_run(ctx, &rows));
      mark("  mkp_shard_run returned");
      if (a.rerun) must(ctx, mkp_shard_rerun(ctx, a.rerun, &rows));   // measurement aid: warm, averaged kernel times in --stats
      if (!a.region_stats.empty()) must(ctx, mkp_stats_add_resident(ctx));   // the rows are still in HBM: this shard's share of every region
      if (!a.localize.empty()) must(ctx, mkp_localize_add_resident(ctx));     // ... and of every window
      if (!a.merge_bedmethyl.empty()) must(ctx, mkp_merge_add_resident(ctx));  // --merge-bedmethyl: joined into the contig's table, not read back
      auto t_w = std::chrono::steady_clock::now();
      out.write(rec.name, rows);
      c.write_ms += ms_since(t_w);
    }
    mark("shard run, rows with the writer");
    c.add_shard(ctx, sp.bp, rows);
  }
}

int run(const Args& a, mkp_ctx* ext_ctx, mkp_run_report* rep) {
  Counters c; c.t_all = std::chrono::steady_clock::now();
  // BAI next to the BAM: only the blocks of the shards (and sampling intervals) this run touches are read and inflated; otherwise
  // the whole file is loaded once.  (inflate threads: --threads only steers the sampling schedule)
  std::unique_ptr<BamSource> src = BamSource::open(a.in_bam, std::max(std::max<unsigned>((unsigned)a.threads, 1u), HostPool::host_cpus()),
      !a.no_index);
  const BamSource& bam = *src;
  c.load_ms = ms_since(c.t_all);
  const Knobs kn;
  const Marks mark{kn.trace, c.t_all};
  mark("BAM opened (header, index)");
  Options o(a, bam);
  const std::vector<Contig>& records = o.records;
  mkp_config cfg; memset(&cfg, 0, sizeof(cfg)); cfg.device = a.device; cfg.tile_positions = a.tile;
  mkp_ctx* ctx = ext_ctx;
  int rc = (a.plan_only || ext_ctx) ? MKP_OK : mkp_ctx_create(&cfg, &ctx);   // --plan-only: shard plan of this rank, no device work
  if (rc != MKP_OK) throw Error(rc, "no usable gfx950 device (libmkpileup has no CPU path)");
  // destroyed last: every object below that runs threads on the context joins them when it dies
  struct OwnedCtx { mkp_ctx* c; ~OwnedCtx() { if (c) mkp_ctx_destroy(c); } } owned_ctx{ext_ctx ? nullptr : ctx};
  const ShardReader reader(a, kn, *src, ctx);
  const bool dev_ingest = reader.dev_ingest;
  const ShardSize size(a, kn, bam, records);
  AheadIngest ahead(reader, ctx, a.hbm_budget_mb, kn);
  Grid g(records.size());
  // One target contig that fits one shard whatever its grid turns out to be: the device ingest of that window starts now, before the
  // reference is read and the grid walked (if the grid's one shard is not this window after all, the ingest is repeated for the plan's)
  if (dev_ingest && a.world == 1 && records.size() == 1 && records[0].length > 0 && !kn.no_early_fetch && size.bp >= records[0].length
      && bam.offset_at(records[0].tid, records[0].end()) - bam.offset_at(records[0].tid, records[0].start) <= size.bytes) {
    g.early_whole = true; g.fetch_early(reader, records[0].tid, records[0].start, records[0].end()); }
  // several target contigs (or the BED records of several contigs), each fitting one shard: all of them are ingested ahead
  if (dev_ingest && !g.early_whole && a.world == 1 && !records.empty() && !kn.no_early_fetch && !kn.no_ahead) ahead.from_contigs(records, o.bf, size);
  o.load_fasta(mark);
  if (o.fb.has_focus() && a.world == 1 && !a.plan_only && a.filter_threshold.empty() && !a.no_filtering) {
    const bool first_shard_early = !g.early_whole && !o.bf && ahead.empty() && !kn.no_early_fetch;
    g.walk = std::async(std::launch::async, [&, first_shard_early]() {
      auto t_focus = std::chrono::steady_clock::now();
      for (size_t ri = 0; ri < records.size(); ri++) {
        g.grid_of[ri] = o.fb.walk(records[ri], a.interval_size, &g.focus_of[ri]); g.grid_done[ri] = 1; g.focus_done[ri] = 1;
        // (--include-bed: the first shard is a merge of records, known only with the plan)
        if (ri == 0 && first_shard_early && !g.grid_of[0].empty()) {
          uint64_t bp; const size_t i1 = size.cut(records[0], g.grid_of[0], 0, &bp);
          g.fetch_early(reader, records[0].tid, g.grid_of[0][0].start, g.grid_of[0][i1 - 1].end);
        }
      }
      g.focus_ms += ms_since(t_focus);
    });
  }
  Plan plan;
  o.kc.per_mod = o.per_mod.data(); o.kc.n_per_mod = (uint32_t)o.per_mod.size();
  EarlyShard early;   // the first shard's records, taken before the loop
  const bool full_mode = a.have_frac && a.sampling_frac >= 1.0;
  const bool want_estimate = a.filter_threshold.empty() && !a.no_filtering && !a.plan_only;
  const bool resident_ok = !o.have_sregion && !a.include_unmapped && !kn.no_resident_sampling;
  // The plan comes before the thresholds — and its shards go ahead — when nothing is gained by waiting for them: several ranks (a rank needs
  // its own shards whatever the thresholds turn out to be, and the others' estimate or all-reduce is time to ingest in), thresholds given,
  // or a full-data estimate, which samples from the shards themselves.
  if (dev_ingest && !g.early_whole && ahead.empty() && !kn.no_ahead && (a.world > 1 || !want_estimate || (full_mode && resident_ok))) {
    build_plan(plan, a, kn, bam, o, g, size, !ahead.empty(), mark); ahead.from_plan(plan.shards, records, o.bf); }
  // thresholds (subcommand.rs:615-638)
  if (!a.filter_threshold.empty()) parse_base_thresholds(a.filter_threshold, &o.kc);
  else if (a.no_filtering || a.plan_only) { o.kc.n_per_mod = 0; }  // MultipleThresholdModCaller::new_passthrough
  else estimate_thresholds(a, kn, bam, o, ctx, g, ahead, plan, size, dev_ingest, resident_ok, early, c, mark);
  c.resident_used = c.resident_used || early.attached;
  mark("thresholds done");
  if (!a.plan_only) must(ctx, mkp_set_caller(ctx, &o.kc));
  g.join_walk();
  Outputs out(a, ctx, o.labels);
  // --region-stats: the regions (contigs by the BAM header's names) and the run-long table in HBM; --region-stats-only: no row read-back
  mkp_region_set rset;
  struct RowFetchGuard { mkp_ctx* c; ~RowFetchGuard() { if (c) { mkp_internal_skip_row_fetch(c, 0); mkp_internal_stats_timing(c, 0, nullptr);
      mkp_internal_localize_timing(c, 0, nullptr); mkp_internal_merge_timing(c, 0, nullptr); } } } fetch_guard{nullptr};
  if (!a.region_stats.empty()) {
    rset = parse_regions_bed(a.region_stats, [&](const std::string& chrom) { return bam.tid_of(chrom); });
    must(ctx, mkp_stats_begin(ctx, rset.regions.data(), (uint32_t)rset.regions.size(), a.region_stats_codes.data(),
        (uint32_t)a.region_stats_codes.size(), a.region_stats_min_cov));
    fetch_guard.c = ctx;
    if (a.stats) must(ctx, mkp_internal_stats_timing(ctx, 1, nullptr));
  }
  // --localize: the same hooks, the windows around the regions' midpoints (contig lengths from the BAM header)
  size_t n_localize_regions = 0;
  if (!a.localize.empty()) {
    uint32_t skipped = 0;
    const mkp_region_set lset = parse_localize_regions_bed(a.localize, [&](const std::string& chrom) { return bam.tid_of(chrom); }, &skipped);
    n_localize_regions = lset.regions.size();
    std::vector<uint64_t> lens(bam.ref_lens.begin(), bam.ref_lens.end());
    must(ctx, mkp_localize_begin(ctx, lset.regions.data(), (uint32_t)lset.regions.size(), lens.data(), (uint32_t)lens.size(), a.localize_window,
        a.localize_stranded, a.localize_stranded_features));
    fetch_guard.c = ctx;
    if (a.stats) must(ctx, mkp_internal_localize_timing(ctx, 1, nullptr));
    if (skipped) mark("  localize: regions BED lines skipped");
  }
  // --merge-bedmethyl: the prior tables go up before the first shard; every shard's rows are then joined where they are
  double merge_upload_ms = 0; uint64_t merge_prior_rows = 0;
  if (!a.merge_bedmethyl.empty()) {
    auto t_m = std::chrono::steady_clock::now();
    std::vector<uint64_t> lens(bam.ref_lens.begin(), bam.ref_lens.end());
    must(ctx, mkp_merge_begin(ctx, lens.data(), (uint32_t)lens.size()));
    fetch_guard.c = ctx;
    if (a.stats) must(ctx, mkp_internal_merge_timing(ctx, 1, nullptr));
    std::vector<const char*> names; for (const std::string& s : bam.ref_names) names.push_back(s.c_str());
    for (const std::string& path : a.merge_bedmethyl) {
      if (Knobs::one("MKP_HOST_BEDMETHYL")) {   // the host reader and mkp_merge_add_rows (the stage's earlier form)
        const mkp_bedmethyl_file prior = read_bedmethyl_text(path);
        merge_prior_rows += prior.n_rows();
        for (size_t k = 0; k < prior.runs.size(); k++) { const mkp_rows rows = prior.rows_of(k);
          must(ctx, mkp_merge_add_rows(ctx, bam.tid_of(prior.runs[k].chrom), &rows)); }
      } else { uint64_t n = 0; must(ctx, mkp_merge_add_file(ctx, path.c_str(), names.data(), (uint32_t)names.size(), &n)); merge_prior_rows += n; }
    }
    merge_upload_ms = ms_since(t_m);
    mark("prior bedMethyl tables uploaded");
  }
  if (a.rows_stay() || !a.merge_bedmethyl.empty()) must(ctx, mkp_internal_skip_row_fetch(ctx, 1));
  build_plan(plan, a, kn, bam, o, g, size, !ahead.empty(), mark);
  // (thresholds known before the plan: the shards go ahead of the loop from here)
  if (ahead.empty() && plan.shards.size() > 1 && !kn.no_ahead) ahead.from_plan(plan.shards, records, o.bf);
  run_shards(a, o, ctx, reader, g, ahead, plan, early, out, c, mark);
  c.load_ms += c.fetch_wait_ms;   // what the shard loop waited for blocks to be read and inflated (the rest overlapped with pack / run / write)
  if (!a.merge_bedmethyl.empty()) {   // the merged contigs, in the BAM header's order, through the writer of a plain run
    uint64_t dropped = 0; double get_ms = 0, wr_ms = 0;
    for (size_t tid = 0; tid < bam.ref_names.size(); tid++) {
      auto t_g = std::chrono::steady_clock::now();
      mkp_rows rows; must(ctx, mkp_merge_get(ctx, (int32_t)tid, &rows, &dropped));
      get_ms += ms_since(t_g);
      auto t_w = std::chrono::steady_clock::now();
      out.write(bam.ref_names[tid], rows);
      wr_ms += ms_since(t_w);
    }
    c.d2h_ms += get_ms; c.write_ms += wr_ms;
    if (dropped) fprintf(stderr, "[mkpileup] bedmethyl merge: %llu rows dropped (beyond their contig's length, or on a contig the BAM header does not list)\n",
        (unsigned long long)dropped);
    if (a.stats) { double ms[2] = {0, 0}; mkp_internal_merge_timing(ctx, 0, ms);
      double in_ms[4] = {0, 0, 0, 0}; uint64_t pieces = 0; mkp_internal_bedmethyl_in_stats(ctx, 1, in_ms, &pieces);
      fprintf(stderr, "[mkpileup] bedmethyl merge: device reader of the priors: file read %.1f ms, upload %.1f, inflate %.1f, parse %.1f (%llu pieces)\n", in_ms[0], in_ms[1],
          in_ms[2], in_ms[3], (unsigned long long)pieces);
      fprintf(stderr, "[mkpileup] bedmethyl merge: %zu prior tables, %llu prior rows, upload + join of the priors %.1f ms; kernels partition %.3f ms, tile + scan + compaction %.3f ms (summed over the adds); merged rows d2h %.1f ms, formatted %.1f ms\n",
          a.merge_bedmethyl.size(), (unsigned long long)merge_prior_rows, merge_upload_ms, ms[0], ms[1], get_ms, wr_ms); }
    mark("merged rows with the writer");
  }
  { auto t_w = std::chrono::steady_clock::now(); out.finish(); c.write_ms += ms_since(t_w); }
  out.close();
  mark("output closed");
  if (!a.region_stats.empty()) {
    auto t_w = std::chrono::steady_clock::now();
    mkp_stats_out table; must(ctx, mkp_stats_get(ctx, &table));
    write_text_file(a.region_stats_out, stats_table_text(rset, table, !a.region_stats_no_header, f32_display));
    c.write_ms += ms_since(t_w);
    if (a.stats) { double ms[2] = {0, 0}; mkp_internal_stats_timing(ctx, 0, ms);
      fprintf(stderr, "[mkpileup] region stats: %zu regions, %u codes; kernels bounds+scan %.3f ms, reduce %.3f ms (summed over the shards)\n",
          rset.regions.size(), table.n_codes, ms[0], ms[1]); }
    mark("region stats table written");
  }
  if (!a.localize.empty()) {
    auto t_w = std::chrono::steady_clock::now();
    mkp_localize_out table; must(ctx, mkp_localize_get(ctx, &table));
    write_text_file(a.localize_out, localize_table_text(table, f32_display));
    c.write_ms += ms_since(t_w);
    if (a.stats) { double ms[2] = {0, 0}; mkp_internal_localize_timing(ctx, 0, ms);
      fprintf(stderr, "[mkpileup] localize: %zu regions, window %u, %u codes; kernels bounds %.3f ms, reduce %.3f ms (summed over the shards)\n",
          n_localize_regions, a.localize_window, table.n_codes, ms[0], ms[1]); }
    mark("localize table written");
  }
  const uint64_t n_rows_out = a.rows_stay() ? c.dev_rows : out.rows();
  if (rep) c.report(rep, n_rows_out, g.focus_ms, o.kc);
  if (a.stats) c.print_stats(a, bam, n_rows_out, g.focus_ms, dev_ingest, ahead);
  return MKP_OK;
}

void parse_args(int argc, const char* const* argv, Args* out, bool need_positional, bool hemi = false) {
  Args& a = *out; std::vector<std::string> pos;
  a.hemi = hemi;
  for (int i = 0; i < argc; i++) {
    std::string s = argv[i];
    auto val = [&]() { if (i + 1 >= argc) throw Error(MKP_E_INVALID, "missing value for " + s); return std::string(argv[++i]); };
    if (hemi && (s == "--preset" || s == "--combine-strands" || s == "--with-header" || s == "--header" || s == "--partition-tag" || s == "--prefix"
        || s == "--bedgraph" || s == "--plan-only" || s.compare(0, 14, "--region-stats") == 0 || s.compare(0, 10, "--localize") == 0
        || s == "--merge-bedmethyl"))
      throw Error(MKP_E_INVALID, "unexpected argument '" + s + "' for pileup-hemi");
    if (hemi && (s == "-o" || s == "--out-bed")) { a.out_bed = val(); continue; }
    if (s == "--region") a.region = val(); else if (s == "--max-depth") a.max_depth = (uint32_t)std::stoul(val());
    else if (s == "-t" || s == "--threads") a.threads = std::stoul(val());
      else if (s == "-i" || s == "--interval-size") a.interval_size = (uint32_t)std::stoul(val());
    else if (s == "--chunk-size" || s == "--queue-size" || s == "--log-filepath") val();
    else if (s == "--seed") { a.have_seed = true; a.seed = std::stoull(val()); }
    else if (s == "-n" || s == "--num-reads") a.num_reads = std::stoul(val()); else if (s == "-f" || s == "--sampling-frac") { a.have_frac = true;
        a.sampling_frac = std::stod(val()); }
    else if (s == "--no-filtering") a.no_filtering = true; else if (s == "-p" || s == "--filter-percentile") a.filter_percentile = std::stof(val());
    else if (s == "--filter-threshold") a.filter_threshold.push_back(val());
        else if (s == "--mod-thresholds" || s == "--mod-threshold") a.mod_thresholds.push_back(val());
    else if (s == "--sample-region") a.sample_region = val();
      else if (s == "--sampling-interval-size") a.sampling_interval_size = (uint32_t)std::stoul(val());
    else if (s == "--include-bed" || s == "--include-positions") a.include_bed = val(); else if (s == "--include-unmapped") a.include_unmapped = true;
    else if (s == "--ignore") a.ignore = val(); else if (s == "--force-allow-implicit") a.force_allow = true;
    else if (s == "--motif") { a.motif_parts.push_back(val()); a.motif_parts.push_back(val()); } else if (s == "--cpg") a.cpg = true;
    else if (s == "--ref" || s == "-r") a.ref_fasta = val(); else if (s == "--mask" || s == "-k") a.mask = true;
      else if (s == "--preset") a.preset = val();
    else if (s == "--combine-mods") a.combine_mods = true; else if (s == "--combine-strands") a.combine_strands = true;
    else if (s == "--edge-filter") a.edge_filter = val(); else if (s == "--invert-edge-filter") a.invert_edge = true;
    else if (s == "--only-tabs" || s == "--suppress-progress") {} else if (s == "--mixed-delim") a.mixed_delim = true;
        else if (s == "--with-header" || s == "--header") a.with_header = true;
    else if (s == "--device") a.device = std::stoi(val()); else if (s == "--gpus-rank") a.rank = (uint32_t)std::stoul(val());
        else if (s == "--gpus-world") a.world = (uint32_t)std::stoul(val());
    else if (s == "--plan-only") a.plan_only = true; else if (s == "--plan-pack-min") a.plan_pack_min = (uint32_t)std::stoul(val());
        else if (s == "--rerun") a.rerun = (uint32_t)std::stoul(val()); else if (s == "--shard-bp") a.shard_bp = std::stoull(val());
        else if (s == "--shard-bytes") { a.shard_bytes = std::max<uint64_t>(1, std::stoull(val())); a.shard_bytes_set = true;
          } else if (s == "--no-index") a.no_index = true;
        else if (s == "--device-inflate") a.device_inflate = true; else if (s == "--host-ingest") a.host_ingest = true;
        else if (s == "--hbm-budget-mb") a.hbm_budget_mb = std::stoull(val());
        else if (s == "--tile") a.tile = (uint32_t)std::stoul(val()); else if (s == "--stats") a.stats = true;
    else if (s == "--partition-tag") a.partition_tags.push_back(val()); else if (s == "--prefix") a.prefix = val();
    else if (s == "--bgzf") a.bgzf = true;
    else if (s == "--bedgraph") a.bedgraph = true;
    else if (s == "--region-stats") a.region_stats = val(); else if (s == "--region-stats-out") a.region_stats_out = val();
    else if (s == "--region-stats-codes") { const std::string v = val();   // comma-delimited, repeatable (ModCodeRepr::parse each)
      for (size_t p0 = 0;;) { const size_t p1 = v.find(',', p0); const std::string one = v.substr(p0, p1 == std::string::npos ? p1 : p1 - p0);
        uint32_t code; if (!parse_code(one, &code)) throw Error(MKP_E_INVALID, "bad mod code '" + one + "' in --region-stats-codes");
        a.region_stats_codes.push_back(code); if (p1 == std::string::npos) break; p0 = p1 + 1; } }
    else if (s == "--region-stats-min-coverage") a.region_stats_min_cov = std::stoull(val());
    else if (s == "--region-stats-no-header") a.region_stats_no_header = true; else if (s == "--region-stats-only") a.region_stats_only = true;
    else if (s == "--localize") a.localize = val(); else if (s == "--localize-out") a.localize_out = val();
    else if (s == "--localize-window") { const std::string v = val();
      if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 9) throw Error(MKP_E_INVALID, "bad --localize-window " + v);
      a.localize_window = (uint32_t)std::stoul(v); a.have_localize_window = true; }
    else if (s == "--localize-stranded") { const std::string v = val(); a.localize_stranded = v == "same" ? 1 : v == "opposite" ? 2 : 0;
      if (!a.localize_stranded) throw Error(MKP_E_INVALID, "--localize-stranded takes same or opposite, not '" + v + "'"); }
    else if (s == "--localize-stranded-features") { const std::string v = val();   // (the reference's value names, and the strand characters)
      a.localize_stranded_features = v == "+" || v == "positive" ? 1 : v == "-" || v == "negative" ? 2 : v == "." || v == "both" ? 3 : 0;
      if (!a.localize_stranded_features) throw Error(MKP_E_INVALID, "--localize-stranded-features takes +, - or ., not '" + v + "'"); }
    else if (s == "--localize-only") a.localize_only = true;
    else if (s == "--merge-bedmethyl") a.merge_bedmethyl.push_back(val());
    else if (!s.empty() && s[0] == '-' && s != "-") throw Error(MKP_E_INVALID, "unknown flag " + s);
    else pos.push_back(s);
  }
  if (need_positional && hemi) { if (pos.size() != 1) throw Error(MKP_E_INVALID, "usage: <in.bam> -o <out.bed> [flags of `modkit pileup-hemi`]");
    a.in_bam = pos[0]; }
  else if (need_positional) { if (pos.size() != 2) throw Error(MKP_E_INVALID, "usage: <in.bam> <out.bed> [flags of `modkit pileup`]");
    a.in_bam = pos[0];
      a.out_bed = pos[1]; }
  else if (!pos.empty()) throw Error(MKP_E_INVALID, "unexpected positional argument " + pos[0]);
  if (a.world == 0 || a.rank >= a.world) throw Error(MKP_E_INVALID, "bad --gpus-rank/--gpus-world");
  if (a.region_stats.empty()) { if (!a.region_stats_out.empty() || !a.region_stats_codes.empty() || a.region_stats_no_header || a.region_stats_only
      || a.region_stats_min_cov != 1) throw Error(MKP_E_INVALID, "the --region-stats-* flags need --region-stats <regions.bed>"); }
  else {
    if (a.region_stats_out.empty()) throw Error(MKP_E_INVALID, "--region-stats needs --region-stats-out <table.tsv>");
    if (!a.partition_tags.empty()) throw Error(MKP_E_INVALID,
        "--region-stats cannot be combined with --partition-tag: the rows of a partitioned run come grouped by key, not in genome order");
    if (a.plan_only) throw Error(MKP_E_INVALID, "--region-stats cannot be combined with --plan-only");
    if (a.region_stats_only && (a.bedgraph || a.bgzf)) throw Error(MKP_E_INVALID, "--region-stats-only writes no rows: drop --bedgraph / --bgzf");
    if (a.world > 1) throw Error(MKP_E_UNSUPPORTED,
        "--region-stats with --gpus-world > 1: the ranks' tables would have to be summed (an all-reduce that is not implemented)");
  }
  if (a.localize.empty()) { if (!a.localize_out.empty() || a.have_localize_window || a.localize_stranded || a.localize_stranded_features
      || a.localize_only) throw Error(MKP_E_INVALID, "the --localize-* flags need --localize <regions.bed>"); }
  else {
    if (a.localize_out.empty()) throw Error(MKP_E_INVALID, "--localize needs --localize-out <table.tsv>");
    if (!a.partition_tags.empty()) throw Error(MKP_E_INVALID,
        "--localize cannot be combined with --partition-tag: the rows of a partitioned run come grouped by key, not in genome order");
    if (a.plan_only) throw Error(MKP_E_INVALID, "--localize cannot be combined with --plan-only");
    if (a.localize_only && (a.bedgraph || a.bgzf)) throw Error(MKP_E_INVALID, "--localize-only writes no rows: drop --bedgraph / --bgzf");
    if (a.localize_window > MKP_LOC_MAX_WINDOW) throw Error(MKP_E_UNSUPPORTED, "--localize-window beyond " + std::to_string(MKP_LOC_MAX_WINDOW));
    if (a.world > 1) throw Error(MKP_E_UNSUPPORTED,
        "--localize with --gpus-world > 1: the ranks' tables would have to be summed (an all-reduce that is not implemented)");
  }
  if (!a.merge_bedmethyl.empty()) {
    if (!a.partition_tags.empty()) throw Error(MKP_E_INVALID,
        "--merge-bedmethyl cannot be combined with --partition-tag: the rows of a partitioned run come grouped by key, not in genome order");
    if (a.bedgraph) throw Error(MKP_E_INVALID, "--merge-bedmethyl cannot be combined with --bedgraph: the merged rows are bedMethyl lines");
    if (!a.region_stats.empty() || !a.localize.empty()) throw Error(MKP_E_INVALID,
        "--merge-bedmethyl cannot be combined with --region-stats / --localize: they reduce the run's own rows, not the merged ones");
    if (a.plan_only) throw Error(MKP_E_INVALID, "--merge-bedmethyl cannot be combined with --plan-only");
    if (a.world > 1) throw Error(MKP_E_UNSUPPORTED,
        "--merge-bedmethyl with --gpus-world > 1: every rank would have to hold the prior tables and the ranks' outputs be joined");
  }
}

}  // namespace

// (tests) the --bedgraph writer alone: rows in, files out — no device involved
extern "C" int mkp_internal_bedgraph_write(const char* dir, const char* prefix, int groupings, const char* const* motif_labels, uint32_t n_labels,
    const char* chrom, const mkp_rows* rows) {
  if (!dir || !chrom || !rows) return MKP_E_INVALID;
  return guarded_status([&]() {
    BedGraphOut bg; bg.dir = dir; bg.prefix = prefix ? prefix : ""; bg.groupings = groupings != 0;
    for (uint32_t k = 0; k < n_labels; k++) bg.labels.push_back(motif_labels[k]);
    bg.write(chrom, *rows); bg.finish();
    return MKP_OK;
  });
}

// `modkit stats`, host halves (include/mkpileup.h): the regions BED and the table, no device involved
extern "C" int mkp_host_parse_regions(const char* bed_path, const char* const* contig_names, uint32_t n_contigs, mkp_region_set** out, char* errbuf,
    size_t errbuf_len) {
  if (!bed_path || !out || (!contig_names && n_contigs)) return fail_into(errbuf, errbuf_len, MKP_E_INVALID, "bad argument");
  *out = nullptr;
  return guarded_buf(errbuf, errbuf_len, [&]() {
    std::map<std::string, int> tids; for (uint32_t k = 0; k < n_contigs; k++) tids.emplace(contig_names[k], (int)k);
    std::unique_ptr<mkp_region_set> set(new mkp_region_set(parse_regions_bed(bed_path, [&](const std::string& chrom) { auto it = tids.find(chrom);
      return it == tids.end() ? -1 : it->second; })));
    *out = set.release();
    return MKP_OK;
  });
}
extern "C" uint32_t mkp_region_set_size(const mkp_region_set* set) { return set ? (uint32_t)set->regions.size() : 0u; }
extern "C" const mkp_region* mkp_region_set_regions(const mkp_region_set* set) { return set ? set->regions.data() : nullptr; }
extern "C" const char* mkp_region_set_chrom(const mkp_region_set* set, uint32_t i) { return set && i < set->chrom.size() ? set->chrom[i].c_str() : nullptr; }
extern "C" const char* mkp_region_set_name(const mkp_region_set* set, uint32_t i) { return set && i < set->name.size() ? set->name[i].c_str() : nullptr; }
extern "C" void mkp_region_set_free(mkp_region_set* set) { delete set; }
extern "C" int mkp_host_parse_localize_regions(const char* bed_path, const char* const* contig_names, uint32_t n_contigs, mkp_region_set** out,
    uint32_t* n_skipped, char* errbuf, size_t errbuf_len) {
  if (!bed_path || !out || (!contig_names && n_contigs)) return fail_into(errbuf, errbuf_len, MKP_E_INVALID, "bad argument");
  *out = nullptr;
  return guarded_buf(errbuf, errbuf_len, [&]() {
    std::map<std::string, int> tids; for (uint32_t k = 0; k < n_contigs; k++) tids.emplace(contig_names[k], (int)k);
    std::unique_ptr<mkp_region_set> set(new mkp_region_set(parse_localize_regions_bed(bed_path, [&](const std::string& chrom) {
      auto it = tids.find(chrom); return it == tids.end() ? -1 : it->second; }, n_skipped)));
    *out = set.release();
    return MKP_OK;
  });
}
extern "C" int mkp_host_parse_genome_sizes(const char* path, mkp_genome_sizes** out, char* errbuf, size_t errbuf_len) {
  if (!path || !out) return fail_into(errbuf, errbuf_len, MKP_E_INVALID, "bad argument");
  *out = nullptr;
  return guarded_buf(errbuf, errbuf_len, [&]() { *out = new mkp_genome_sizes(parse_genome_sizes(path)); return MKP_OK; });
}
extern "C" uint32_t mkp_genome_sizes_size(const mkp_genome_sizes* z) { return z ? (uint32_t)z->name.size() : 0u; }
extern "C" const char* mkp_genome_sizes_name(const mkp_genome_sizes* z, uint32_t i) { return z && i < z->name.size() ? z->name[i].c_str() : nullptr; }
extern "C" uint64_t mkp_genome_sizes_length(const mkp_genome_sizes* z, uint32_t i) { return z && i < z->length.size() ? z->length[i] : 0ull; }
extern "C" void mkp_genome_sizes_free(mkp_genome_sizes* z) { delete z; }
extern "C" int mkp_host_localize_table(const mkp_localize_out* counts, const char* out_path) {
  if (!counts || !out_path) return MKP_E_INVALID;
  return guarded_status([&]() { write_text_file(out_path, localize_table_text(*counts, f32_display)); return MKP_OK; });
}
extern "C" int mkp_host_stats_table(const mkp_region_set* set, const mkp_stats_out* counts, int with_header, const char* out_path) {
  if (!set || !counts || !out_path) return MKP_E_INVALID;
  return guarded_status([&]() { write_text_file(out_path, stats_table_text(*set, *counts, with_header != 0, f32_display)); return MKP_OK; });
}

// `modkit bedmethyl merge`, host half (include/mkpileup.h): the host reader (plain text or BGZF), no device involved
extern "C" int mkp_host_read_bedmethyl(const char* path, mkp_bedmethyl_file** out, char* errbuf, size_t errbuf_len) {
  if (!path || !out) return fail_into(errbuf, errbuf_len, MKP_E_INVALID, "bad argument");
  *out = nullptr;
  return guarded_buf(errbuf, errbuf_len, [&]() { *out = new mkp_bedmethyl_file(read_bedmethyl_text(path)); return MKP_OK; });
}
extern "C" uint32_t mkp_bedmethyl_file_runs(const mkp_bedmethyl_file* f) { return f ? (uint32_t)f->runs.size() : 0u; }
extern "C" const char* mkp_bedmethyl_file_chrom(const mkp_bedmethyl_file* f, uint32_t run) {
  return f && run < f->runs.size() ? f->runs[run].chrom.c_str() : nullptr; }
extern "C" int mkp_bedmethyl_file_rows(const mkp_bedmethyl_file* f, uint32_t run, mkp_rows* out) {
  if (!f || !out || run >= f->runs.size()) return MKP_E_INVALID;
  *out = f->rows_of(run); return MKP_OK;
}
extern "C" void mkp_bedmethyl_file_free(mkp_bedmethyl_file* f) { delete f; }

// `mkpileup bedmethyl merge` (EntryMergeBedMethyl::run, src/bedmethyl_util/subcommands.rs:198-371): the inputs are read on the device and their
// contig runs joined one after the other (mkp_merge_add_file), the merged contigs come back in the order of the sizes file.  --mixed-delim and --header are parsed by the
// reference and never used: they are not offered.
extern "C" int mkp_bedmethyl_merge_main(int argc, const char* const* argv, uint64_t* n_written, uint64_t* n_dropped, char* errbuf, size_t errbuf_len) {
  return guarded_buf(errbuf, errbuf_len, [&]() {
    std::vector<std::string> inputs; std::string sizes_path, out_path; bool force = false, bgzf = false, stats = false; int device = 0;
    for (int i = 0; i < argc; i++) {
      const std::string s = argv[i];
      auto val = [&]() { if (i + 1 >= argc) throw Error(MKP_E_INVALID, "missing value for " + s); return std::string(argv[++i]); };
      if (s == "-g" || s == "--genome-sizes") sizes_path = val(); else if (s == "-o" || s == "--out-bed") out_path = val();
      else if (s == "-f" || s == "--force") force = true; else if (s == "--bgzf") bgzf = true; else if (s == "--stats") stats = true;
      else if (s == "--device") device = std::stoi(val());
      else if (s == "-t" || s == "--threads" || s == "--io-threads" || s == "--chunk-size" || s == "--interval-size" || s == "--queue-size"
          || s == "--log-filepath") val();   // (the reference's compute options: nothing here is sized by them)
      else if (!s.empty() && s[0] == '-' && s != "-") throw Error(MKP_E_INVALID, "unexpected argument '" + s + "' for bedmethyl merge");
      else inputs.push_back(s);
    }
    if (inputs.size() < 2) throw Error(MKP_E_INVALID, "usage: bedmethyl merge <a.bed> <b.bed> [..] -g <sizes.tsv> -o <out.bed> [--force] [--bgzf]");
    if (sizes_path.empty()) throw Error(MKP_E_INVALID, "bedmethyl merge needs -g <sizes.tsv>");
    if (out_path.empty()) throw Error(MKP_E_INVALID, "bedmethyl merge needs -o <out.bed>");
    const bool to_stdout = out_path == "-" || out_path == "stdout";
    if (bgzf && to_stdout) throw Error(MKP_E_INVALID, "--bgzf writes a file and its index: it needs an output path");
    auto t_all = std::chrono::steady_clock::now();
    const mkp_genome_sizes sizes = parse_genome_sizes(sizes_path);
    // MKP_HOST_BEDMETHYL=1: the host reader and mkp_merge_add_rows (the stage's earlier form); otherwise the device reader takes each file
    const bool host_read = Knobs::one("MKP_HOST_BEDMETHYL");
    std::vector<mkp_bedmethyl_file> files;
    if (host_read) for (auto& p : inputs) files.push_back(read_bedmethyl_text(p));
    else for (auto& p : inputs) { std::ifstream f(p, std::ios::binary); if (!f) throw Error(MKP_E_IO, "failed to open bedMethyl " + p); }
    const double read_ms = ms_since(t_all);
    // the output is opened before any device work, as the reference opens it (File::create_new without --force)
    RowWriter wr;
    if (to_stdout) wr.f = stdout;
    else {
      struct stat sb;
      if (!force && stat(out_path.c_str(), &sb) == 0) throw Error(MKP_E_IO, "refusing to overwrite " + out_path + " without --force");
      wr.f = fopen(out_path.c_str(), "w+");
      if (!wr.f) throw Error(MKP_E_IO, "failed to make output file " + out_path);
    }
    struct CloseFile { FILE* f; ~CloseFile() { if (f && f != stdout) fclose(f); } } close_file{wr.f};
    if (bgzf) { wr.bz.reset(new BgzfTabixSink()); wr.bz->f = wr.f; wr.bz->index_path = out_path + ".tbi"; }
    mkp_config cfg; memset(&cfg, 0, sizeof(cfg)); cfg.device = device;
    mkp_ctx* ctx = nullptr;
    if (mkp_ctx_create(&cfg, &ctx) != MKP_OK) throw Error(MKP_E_DEVICE, "no usable gfx950 device (libmkpileup has no CPU path)");
    struct OwnedCtx { mkp_ctx* c; ~OwnedCtx() { mkp_ctx_destroy(c); } } owned{ctx};
    auto t_dev = std::chrono::steady_clock::now();
    must(ctx, mkp_merge_begin(ctx, sizes.length.data(), (uint32_t)sizes.length.size()));
    if (stats) must(ctx, mkp_internal_merge_timing(ctx, 1, nullptr));
    if (host_read) {
      std::map<std::string, int32_t> tid_of; for (size_t k = 0; k < sizes.name.size(); k++) tid_of.emplace(sizes.name[k], (int32_t)k);
      for (const mkp_bedmethyl_file& f : files) for (size_t k = 0; k < f.runs.size(); k++) {
        auto it = tid_of.find(f.runs[k].chrom); const mkp_rows rows = f.rows_of(k);
        must(ctx, mkp_merge_add_rows(ctx, it == tid_of.end() ? -1 : it->second, &rows));
      }
    } else {
      std::vector<const char*> names; for (const std::string& s : sizes.name) names.push_back(s.c_str());
      for (auto& p : inputs) must(ctx, mkp_merge_add_file(ctx, p.c_str(), names.data(), (uint32_t)names.size(), nullptr));
    }
    const double add_ms = ms_since(t_dev);
    uint64_t dropped = 0;
    auto t_out = std::chrono::steady_clock::now();
    for (size_t tid = 0; tid < sizes.name.size(); tid++) {
      mkp_rows rows; must(ctx, mkp_merge_get(ctx, (int32_t)tid, &rows, &dropped));
      wr.write(sizes.name[tid], rows);
    }
    wr.finish();
    if (dropped) fprintf(stderr, "[mkpileup] bedmethyl merge: %llu rows dropped (beyond their contig's length, or on a contig the sizes do not list)\n",
        (unsigned long long)dropped);
    if (stats) { double ms[2] = {0, 0}; mkp_internal_merge_timing(ctx, 0, ms);
      // the read stage: the host reader's wall time, or the device reader's four steps (the join's kernels run between its pieces)
      double in_ms[4] = {0, 0, 0, 0}; uint64_t pieces = 0; mkp_internal_bedmethyl_in_stats(ctx, 1, in_ms, &pieces);
      const double stage_ms = host_read ? read_ms : in_ms[0] + in_ms[1] + in_ms[2] + in_ms[3];
      std::string ov; for (char** e = ::environ; e && *e; e++) if (!strncmp(*e, "MKP_", 4)) { ov += ' '; ov += *e; }
      fprintf(stderr, "[mkpileup] bedmethyl merge: %zu inputs, rows written=%llu dropped=%llu; reader=%s read_stage_ms=%.1f (file read %.1f, upload %.1f, inflate %.1f, parse %.1f; %llu pieces) read_ms=%.1f upload+join_ms=%.1f (kernels partition %.3f ms, tile + scan + compaction %.3f ms) d2h+write_ms=%.1f total_ms=%.1f env overrides:%s\n",
          inputs.size(), (unsigned long long)wr.n, (unsigned long long)dropped, host_read ? "host" : "device", stage_ms, host_read ? read_ms : in_ms[0],
          in_ms[1], in_ms[2], in_ms[3], (unsigned long long)pieces, read_ms, add_ms, ms[0], ms[1], ms_since(t_out), ms_since(t_all), ov.c_str()); }
    if (n_written) *n_written = wr.n;
    if (n_dropped) *n_dropped = dropped;
    return MKP_OK;
  });
}

// `modkit dmr pair`, host halves (include/mkpileup.h): the regions BED, the score and the table, no device involved
extern "C" int mkp_host_parse_dmr_regions(const char* bed_path, const char* const* contig_names, uint32_t n_contigs, mkp_region_set** out, char* errbuf,
    size_t errbuf_len) {
  if (!bed_path || !out || (!contig_names && n_contigs)) return fail_into(errbuf, errbuf_len, MKP_E_INVALID, "bad argument");
  *out = nullptr;
  return guarded_buf(errbuf, errbuf_len, [&]() {
    std::map<std::string, int> tids; for (uint32_t k = 0; k < n_contigs; k++) tids.emplace(contig_names[k], (int)k);
    std::unique_ptr<mkp_region_set> set(new mkp_region_set(parse_dmr_regions_bed(bed_path, [&](const std::string& chrom) { auto it = tids.find(chrom);
      return it == tids.end() ? -1 : it->second; })));
    *out = set.release();
    return MKP_OK;
  });
}
extern "C" int mkp_host_dmr_judge(const mkp_dmr_out* counts, double* score, uint8_t* state) {
  if (!counts || !score || !state) return MKP_E_INVALID;
  return guarded_status([&]() { dmr_judge(*counts, score, state); return MKP_OK; });
}
extern "C" int mkp_host_dmr_table(const mkp_region_set* set, const mkp_dmr_out* counts, int with_header, const char* out_path) {
  if (!set || !counts || !out_path) return MKP_E_INVALID;
  return guarded_status([&]() {
    if (counts->n_regions != set->regions.size()) throw Error(MKP_E_INVALID, "the counts are not those of this region set");
    write_text_file(out_path, dmr_table_text(*set, *counts, with_header != 0, f32_display)); return MKP_OK; });
}

// `mkpileup dmr pair` (PairwiseDmr::run with --regions-bed, src/dmr/subcommands.rs:371-560) in stages: arguments, regions, reference, the two
// tables through the device reader (mkp_dmr_add_file), score and text.
namespace {

struct DmrArgs {
  std::vector<std::string> a, b, assign; std::string regions, ref, out, missing = "warn", bases;
  bool force = false, header = false, mask = false, stats = false, segment = false; uint64_t min_cov = 0; int device = 0;
};

DmrArgs parse_dmr_args(int argc, const char* const* argv) {
  DmrArgs d;
  for (int i = 0; i < argc; i++) {
    const std::string s = argv[i];
    auto val = [&]() { if (i + 1 >= argc) throw Error(MKP_E_INVALID, "missing value for " + s); return std::string(argv[++i]); };
    if (s == "-a") d.a.push_back(val()); else if (s == "-b") d.b.push_back(val());
    else if (s == "-r" || s == "--regions-bed") d.regions = val(); else if (s == "--ref") d.ref = val();
    else if (s == "-o" || s == "--out-path") d.out = val(); else if (s == "-f" || s == "--force") d.force = true;
    else if (s == "--header" || s == "--with-header") d.header = true; else if (s == "-k" || s == "--mask") d.mask = true;
    else if (s == "-m" || s == "--base") { const std::string v = val();
      if (v.size() != 1) throw Error(MKP_E_INVALID, "modified base needs to be A, C, G, or T.");
      d.bases += v; }
    else if (s == "--assign-code") d.assign.push_back(val());
    else if (s == "--min-valid-coverage") d.min_cov = std::stoull(val()); else if (s == "--missing") d.missing = val();
    else if (s == "--segment") { d.segment = true; val(); }
    else if (s == "--device") d.device = std::stoi(val()); else if (s == "--stats") d.stats = true;
    else if (s == "-t" || s == "--threads" || s == "--io-threads" || s == "--batch-size" || s == "--log-filepath" || s == "--index-a" || s == "--index-b")
      val();   // (the reference's compute options and tabix indices: nothing here is sized by them, no index is read)
    else if (s == "--suppress-progress") continue;
    else throw Error(MKP_E_INVALID, "unexpected argument '" + s + "' for dmr pair");
  }
  if (d.a.empty() || d.b.empty()) throw Error(MKP_E_INVALID, "need to provide at least 1 'a' sample and 'b' sample");
  if (d.segment) throw Error(MKP_E_UNSUPPORTED, "--segment (single-site segmentation) is not offered: dmr pair scores the regions of -r");
  if (d.regions.empty()) throw Error(MKP_E_UNSUPPORTED, "single-site mode (dmr pair without -r / --regions-bed) is not offered: give the regions with -r");
  if (d.a.size() > 1 || d.b.size() > 1) throw Error(MKP_E_UNSUPPORTED,
      "in order to perform multiple comparisons over regions use modkit dmr multi (which is not offered: one -a and one -b)");
  if (d.ref.empty()) throw Error(MKP_E_INVALID, "the following required arguments were not provided: --ref <REFERENCE_FASTA>");
  if (d.bases.empty()) throw Error(MKP_E_INVALID, "need to specify at least 1 modified base");
  for (char b : d.bases) if (!strchr("ACGT", b)) throw Error(MKP_E_INVALID, "modified base needs to be A, C, G, or T.");
  if (d.missing != "quiet" && d.missing != "warn" && d.missing != "fail") throw Error(MKP_E_INVALID, "--missing takes quiet, warn or fail");
  return d;
}

// MOD_CODE_TO_DNA_BASE, then the --assign-code entries (parse_raw_assignments, subcommands.rs:302-352): a later entry replaces an earlier one
void dmr_code_lookup(const DmrArgs& d, std::vector<uint32_t>* codes, std::vector<uint8_t>* bases) {
  for (const DmrLookupEntry& e : dmr_default_lookup()) { codes->push_back(e.code); bases->push_back(e.base); }
  for (const std::string& raw : d.assign) {
    const size_t colon = raw.find(':');
    const char* base = colon != std::string::npos && raw.find(':', colon + 1) == std::string::npos && raw.size() == colon + 2
        ? strchr("ACGT", raw[colon + 1]) : nullptr;
    uint32_t code = 0;
    if (!base || !raw[colon + 1] || !parse_code(raw.substr(0, colon), &code)) throw Error(MKP_E_INVALID, "invalid assignment " + raw
        + ", should be <code>:<DNA>, such as m:C");
    codes->push_back(code); bases->push_back((uint8_t)(base - "ACGT"));
  }
}

// the regions, tids = their chroms in order of first appearance
struct DmrRegions { mkp_region_set set; std::vector<std::string> chroms; };
DmrRegions dmr_load_regions(const std::string& path) {
  DmrRegions R; std::map<std::string, int> tids;
  R.set = parse_dmr_regions_bed(path, [&](const std::string& chrom) {
    auto it = tids.find(chrom);
    if (it == tids.end()) { it = tids.emplace(chrom, (int)R.chroms.size()).first; R.chroms.push_back(chrom); }
    return it->second; });
  return R;
}

// per contig of the regions that the FASTA holds: the bytes from its lowest region start to its highest region end, once
void dmr_upload_reference(mkp_ctx* ctx, const DmrRegions& R, const Fasta& fasta) {
  for (size_t tid = 0; tid < R.chroms.size(); tid++) {
    const FastaSeq* seq = fasta.get(R.chroms[tid]);
    if (!seq) continue;
    uint32_t lo = 0xffffffffu, hi = 0;
    for (const mkp_region& g : R.set.regions) if (g.tid == (int32_t)tid) {
      if (g.end > seq->size()) throw Error(MKP_E_INVALID, "region " + R.chroms[tid] + ":" + std::to_string(g.start) + "-" + std::to_string(g.end)
          + " ends beyond the contig in the reference FASTA (" + std::to_string(seq->size()) + " bases)");
      lo = std::min(lo, g.start); hi = std::max(hi, g.end);
    }
    if (hi < lo) hi = lo;
    must(ctx, mkp_dmr_set_reference(ctx, (int32_t)tid, (const uint8_t*)seq->data() + lo, lo, hi - lo));
  }
}

// MKP_HOST_BEDMETHYL=1: the host reader and mkp_dmr_add_rows; otherwise the device reader takes the file
void dmr_read_table(mkp_ctx* ctx, int sample, const std::string& path, const DmrRegions& R, bool host_read) {
  if (!host_read) {
    std::vector<const char*> names; for (const std::string& s : R.chroms) names.push_back(s.c_str());
    must(ctx, mkp_dmr_add_file(ctx, sample, path.c_str(), names.data(), (uint32_t)names.size(), nullptr));
    return;
  }
  const mkp_bedmethyl_file f = read_bedmethyl_text(path);
  for (size_t k = 0; k < f.runs.size(); k++) {
    const auto it = std::find(R.chroms.begin(), R.chroms.end(), f.runs[k].chrom);
    if (it == R.chroms.end()) continue;
    const mkp_rows rows = f.rows_of(k);
    must(ctx, mkp_dmr_add_rows(ctx, sample, (int32_t)(it - R.chroms.begin()), &rows));
  }
}

// RoiIter::new (src/dmr/util.rs:180-248): a region on a contig that a table lacks is dropped, with a word (warn) or fatally (fail)
void dmr_handle_missing(const DmrArgs& d, const DmrRegions& R, const mkp_dmr_out& t) {
  std::set<std::string> said; uint32_t kept = 0;
  for (uint32_t r = 0; r < t.n_regions; r++) {
    if (t.contig_has_rows[0][r] && t.contig_has_rows[1][r]) { kept++; continue; }
    const std::string which = t.contig_has_rows[1][r] ? "a" : "'a' and 'b'";
    if (d.missing == "fail") throw Error(MKP_E_INVALID, "chrom " + R.set.chrom[r] + " is missing from " + which + " bedMethyl index, fatal error");
    if (d.missing == "warn" && said.insert(R.set.chrom[r]).second) fprintf(stderr, "[mkpileup] dmr pair: chrom %s is missing from %s bedMethyl, discarding\n",
        R.set.chrom[r].c_str(), which.c_str());
  }
  if (!kept) throw Error(MKP_E_INVALID, "no valid regions in input");
}

}  // namespace

extern "C" int mkp_dmr_pair_main(int argc, const char* const* argv, uint64_t* n_written, char* errbuf, size_t errbuf_len) {
  if (n_written) *n_written = 0;
  return guarded_buf(errbuf, errbuf_len, [&]() {
    const DmrArgs d = parse_dmr_args(argc, argv);
    std::vector<uint32_t> codes; std::vector<uint8_t> code_bases; dmr_code_lookup(d, &codes, &code_bases);
    const bool to_stdout = d.out.empty() || d.out == "-" || d.out == "stdout";
    struct stat sb;
    if (!to_stdout && !d.force && stat(d.out.c_str(), &sb) == 0) throw Error(MKP_E_IO, "refusing to overwrite existing file " + d.out);
    auto t_all = std::chrono::steady_clock::now();
    const DmrRegions R = dmr_load_regions(d.regions);
    const Fasta fasta = Fasta::load(d.ref);
    const double load_ms = ms_since(t_all);
    mkp_config cfg; memset(&cfg, 0, sizeof(cfg)); cfg.device = d.device;
    mkp_ctx* ctx = nullptr;
    if (mkp_ctx_create(&cfg, &ctx) != MKP_OK) throw Error(MKP_E_DEVICE, "no usable gfx950 device (libmkpileup has no CPU path)");
    struct OwnedCtx { mkp_ctx* c; ~OwnedCtx() { mkp_ctx_destroy(c); } } owned{ctx};
    must(ctx, mkp_dmr_begin(ctx, R.set.regions.data(), (uint32_t)R.set.regions.size(), d.bases.data(), (uint32_t)d.bases.size(), codes.data(),
        code_bases.data(), (uint32_t)codes.size(), d.min_cov, d.mask ? 1 : 0));
    if (d.stats) must(ctx, mkp_internal_dmr_timing(ctx, 1, nullptr));
    auto t_ref = std::chrono::steady_clock::now();
    dmr_upload_reference(ctx, R, fasta);
    const double ref_ms = ms_since(t_ref);
    auto t_read = std::chrono::steady_clock::now();
    const bool host_read = Knobs::one("MKP_HOST_BEDMETHYL");
    dmr_read_table(ctx, 0, d.a[0], R, host_read);
    dmr_read_table(ctx, 1, d.b[0], R, host_read);
    const double read_ms = ms_since(t_read);
    auto t_out = std::chrono::steady_clock::now();
    mkp_dmr_out t; must(ctx, mkp_dmr_get(ctx, &t));
    dmr_handle_missing(d, R, t);
    const std::string text = dmr_table_text(R.set, t, d.header, f32_display);
    if (to_stdout) { if (fwrite(text.data(), 1, text.size(), stdout) != text.size()) throw Error(MKP_E_IO, "short write on stdout"); fflush(stdout); }
    else write_text_file(d.out, text);
    uint64_t written = 0; for (uint32_t r = 0; r < t.n_regions; r++) if (t.state[r] == MKP_DMR_WRITTEN) written++;
    if (n_written) *n_written = written;
    if (d.stats) { double ms[2] = {0, 0}; mkp_internal_dmr_timing(ctx, 0, ms);
      double in_ms[4] = {0, 0, 0, 0}; uint64_t pieces = 0; mkp_internal_bedmethyl_in_stats(ctx, 1, in_ms, &pieces);
      fprintf(stderr, "[mkpileup] dmr pair: %u regions, written=%llu; reader=%s regions+fasta_ms=%.1f reference_upload_ms=%.1f read_ms=%.1f (file read %.1f, upload %.1f, inflate %.1f, parse %.1f; %llu pieces) kernels: bounds+scan %.3f ms, reduce %.3f ms; score+text_ms=%.1f total_ms=%.1f\n",
          t.n_regions, (unsigned long long)written, host_read ? "host" : "device", load_ms, ref_ms, read_ms, in_ms[0], in_ms[1], in_ms[2], in_ms[3],
          (unsigned long long)pieces, ms[0], ms[1], ms_since(t_out), ms_since(t_all)); }
    return MKP_OK;
  });
}

// ---- `mkpileup dmr sites` = `modkit dmr pair` without -r (SingleSiteDmrAnalysis::run, src/dmr/single_site.rs) in stages: arguments,
// reference, the two tables through the device reader (mkp_dmr_sites_add_file), the device stages (mkp_dmr_sites_get) and the text.  It is
// not reached through `dmr pair` because that command's refusal of a run without -r is pinned by the suite.
extern "C" int mkp_host_dmr_site_score(const uint64_t* a_mod, uint32_t a_has, uint64_t a_total, const uint64_t* b_mod, uint32_t b_has, uint64_t b_total,
    uint32_t n_codes, double prior_alpha, double prior_beta, double delta, const uint32_t max_coverages[2], double values[5], int* failed) {
  if ((!a_mod || !b_mod) && n_codes) return MKP_E_INVALID;
  if (!max_coverages || !values || !failed || n_codes > MKP_DMR_SITE_MAX_CODES) return MKP_E_INVALID;
  return guarded_status([&]() {
    const MkpDmrSiteMath M = dmr_site_math(prior_alpha, prior_beta, delta, max_coverages);
    *failed = dmr_site_score(a_mod, a_has, a_total, b_mod, b_has, b_total, n_codes, M, values) ? 0 : 1;
    return MKP_OK; });
}
extern "C" int mkp_host_dmr_sites_batches(const uint64_t* contig_len, const uint32_t* window_counts, uint32_t n_contigs, uint64_t interval_size,
    mkp_dmr_sites_batch* entries, uint64_t cap, uint64_t* n_batches) {
  if ((!contig_len || !window_counts) && n_contigs) return MKP_E_INVALID;
  if (!interval_size || (!entries && cap)) return MKP_E_INVALID;
  int n = 0;
  const int rc = guarded_status([&]() {
    std::vector<mkp_dmr_sites_batch> plan;
    const uint64_t nb = dmr_sites_plan(contig_len, window_counts, n_contigs, interval_size, &plan);
    for (size_t e = 0; e < plan.size() && e < cap; e++) entries[e] = plan[e];
    if (n_batches) *n_batches = nb;
    if (plan.size() > 0x7fffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^31 - 1 batch entries");
    n = (int)plan.size();
    return MKP_OK; });
  return rc == MKP_OK ? n : rc;
}
extern "C" int mkp_host_dmr_sites_gauss_legendre(double nodes[16], double weights[16]) {
  if (!nodes || !weights) return MKP_E_INVALID;
  dmr_gauss_legendre(nodes, weights);
  return MKP_OK;
}

namespace {
// the table in pieces on the host pool (30 000 f64 Display lines take 80 ms on one thread), joined in order
std::string dmr_sites_table_text(const mkp_dmr_sites_out& t, const char* const* contig_names, bool header) {
  const uint64_t piece = 8192, np = (t.n_sites + piece - 1) / piece;
  std::vector<std::string> parts((size_t)np);
  HostPool::get().parallel((size_t)np, [&](size_t i) { dmr_sites_rows_text(parts[i], t, contig_names, i * piece, std::min<uint64_t>(t.n_sites, (i + 1) * piece),
      f32_display); });
  size_t total = 0; for (const std::string& p : parts) total += p.size();
  std::string s; s.reserve(total + 256);
  if (header) s = dmr_sites_header();
  for (const std::string& p : parts) s += p;
  return s;
}

struct DmrSitesArgs {
  std::vector<std::string> a, b, assign; std::string ref, out, bases, regions;
  bool force = false, header = false, mask = false, stats = false, segment = false, cap = false, have_prior = false, have_max = false, have_n = false, have_batch = false;
  uint64_t min_cov = 0, n_sample = 10042, interval = 100000, batch_size = 0, threads = 4; double prior[2] = {0.55, 0.55}, delta = 0.05;
  uint32_t max_cov[2] = {0, 0}; int device = 0;
};

// replicates: the command takes several -a / -b (`dmr replicates`); otherwise a second one is refused (`dmr sites`)
DmrSitesArgs parse_dmr_sites_args(int argc, const char* const* argv, bool replicates = false) {
  const std::string cmd = replicates ? "dmr replicates" : "dmr sites";
  DmrSitesArgs d;
  for (int i = 0; i < argc; i++) {
    const std::string s = argv[i];
    auto val = [&]() { if (i + 1 >= argc) throw Error(MKP_E_INVALID, "missing value for " + s); return std::string(argv[++i]); };
    auto num = [&](const std::string& v) { try { size_t used = 0; const double x = std::stod(v, &used); if (used != v.size()) throw 0; return x; }
      catch (...) { throw Error(MKP_E_INVALID, "invalid value '" + v + "' for " + s); } };
    auto whole = [&](const std::string& v) { try { size_t used = 0; if (v.empty() || v[0] == '-') throw 0; const uint64_t x = std::stoull(v, &used);
        if (used != v.size()) throw 0; return x; }
      catch (...) { throw Error(MKP_E_INVALID, "invalid value '" + v + "' for " + s); } };
    if (s == "-a") d.a.push_back(val()); else if (s == "-b") d.b.push_back(val());
    else if (s == "-r" || s == "--regions-bed") d.regions = val(); else if (s == "--ref") d.ref = val();
    else if (s == "-o" || s == "--out-path") d.out = val(); else if (s == "-f" || s == "--force") d.force = true;
    else if (s == "--header" || s == "--with-header") d.header = true; else if (s == "-k" || s == "--mask") d.mask = true;
    else if (s == "-m" || s == "--base") { const std::string v = val();
      if (v.size() != 1) throw Error(MKP_E_INVALID, "modified base needs to be A, C, G, or T.");
      d.bases += v; }
    else if (s == "--assign-code") d.assign.push_back(val());
    else if (s == "--min-valid-coverage") d.min_cov = whole(val());
    else if (s == "--prior") { d.prior[0] = num(val()); d.prior[1] = num(val()); d.have_prior = true; }
    else if (s == "--delta") d.delta = num(val());
    else if (s == "--max-coverages") { for (int k = 0; k < 2; k++) { const uint64_t v = whole(val()); d.max_cov[k] = (uint32_t)std::min<uint64_t>(v, 0xffffffffu); }
      d.have_max = true; }
    else if (s == "-N" || s == "--n-sample-records") { d.n_sample = whole(val()); d.have_n = true; }
    else if (s == "--cap-coverages") d.cap = true;   // (dmr sites: one sample a side, nothing to cap)
    else if (s == "-i" || s == "--interval-size") d.interval = whole(val());
    else if (s == "--batch-size") { d.batch_size = whole(val()); d.have_batch = true; }
    else if (s == "-t" || s == "--threads") d.threads = whole(val());
    else if (s == "--segment") { d.segment = true; val(); }
    else if (s == "--device") d.device = std::stoi(val()); else if (s == "--stats") d.stats = true;
    else if (s == "--io-threads" || s == "--log-filepath" || s == "--index-a" || s == "--index-b" || s == "--missing")
      val();   // (the reference's tabix indices and io threads: no index is read)
    else if (s == "--suppress-progress") continue;
    else throw Error(MKP_E_INVALID, "unexpected argument '" + s + "' for " + cmd);
  }
  if (d.a.empty() || d.b.empty()) throw Error(MKP_E_INVALID, "need to provide at least 1 'a' sample and 'b' sample");
  if (!d.regions.empty()) throw Error(MKP_E_INVALID, "-r / --regions-bed is the region form: use dmr pair (" + cmd + " scores every site of the tables)");
  if (d.segment) throw Error(MKP_E_UNSUPPORTED, "--segment (single-site segmentation) is not offered");
  if (!replicates && (d.a.size() > 1 || d.b.size() > 1)) throw Error(MKP_E_UNSUPPORTED,
      "replicates (more than one -a or -b: balanced columns and per-replicate p-values) are not offered by dmr sites: use dmr replicates");
  if (d.a.size() > MKP_DMR_REPS_MAX_SIDE || d.b.size() > MKP_DMR_REPS_MAX_SIDE) throw Error(MKP_E_UNSUPPORTED, "dmr replicates holds at most "
      + std::to_string(MKP_DMR_REPS_MAX_SIDE) + " tables a side (" + std::to_string(d.a.size()) + " -a, " + std::to_string(d.b.size()) + " -b)");
  if (d.ref.empty()) throw Error(MKP_E_INVALID, "the following required arguments were not provided: --ref <REFERENCE_FASTA>");
  if (d.bases.empty()) throw Error(MKP_E_INVALID, "need to specify at least 1 modified base");
  for (char b : d.bases) if (!strchr("ACGT", b)) throw Error(MKP_E_INVALID, "modified base needs to be A, C, G, or T.");
  if (d.have_prior && d.prior[0] + d.prior[1] < 1.0) throw Error(MKP_E_INVALID, "alpha + beta must be > 1.0 for numerical stability");
  if (d.have_max && d.have_n) throw Error(MKP_E_INVALID,
      "the argument '--max-coverages <MAX_COVERAGES> <MAX_COVERAGES>' cannot be used with '--n-sample-records <N_SAMPLE_RECORDS>'");
  if (!d.have_batch) d.batch_size = (uint64_t)std::floor(1.5 * (double)d.threads);
  return d;
}
}  // namespace

extern "C" int mkp_host_dmr_sites_table(const mkp_dmr_sites_out* sites, const char* const* contig_names, uint32_t n_contigs, int with_header,
    const char* out_path) {
  if (!sites || !out_path || (!contig_names && n_contigs)) return MKP_E_INVALID;
  return guarded_status([&]() {
    for (uint64_t i = 0; i < sites->n_sites; i++) if (sites->tid[i] < 0 || (uint32_t)sites->tid[i] >= n_contigs) throw Error(MKP_E_INVALID,
        "site " + std::to_string(i) + " lies on a contig without a name");
    write_text_file(out_path, dmr_sites_table_text(*sites, contig_names, with_header != 0)); return MKP_OK; });
}

extern "C" int mkp_dmr_sites_main(int argc, const char* const* argv, uint64_t* n_written, char* errbuf, size_t errbuf_len) {
  if (n_written) *n_written = 0;
  return guarded_buf(errbuf, errbuf_len, [&]() {
    const DmrSitesArgs d = parse_dmr_sites_args(argc, argv);
    std::vector<uint32_t> codes; std::vector<uint8_t> code_bases;
    { DmrArgs lookup_args; lookup_args.assign = d.assign; dmr_code_lookup(lookup_args, &codes, &code_bases); }
    const bool to_stdout = d.out.empty() || d.out == "-" || d.out == "stdout";
    struct stat sb;
    if (!to_stdout && !d.force && stat(d.out.c_str(), &sb) == 0) throw Error(MKP_E_IO, "refusing to overwrite existing file " + d.out);
    auto t_all = std::chrono::steady_clock::now();
    const Fasta fasta = Fasta::load(d.ref);
    const double load_ms = ms_since(t_all);
    std::vector<std::string> names; std::vector<const char*> name_ptrs;
    for (const auto& kv : fasta.seqs) names.push_back(kv.first);
    for (const std::string& s : names) name_ptrs.push_back(s.c_str());
    mkp_config cfg; memset(&cfg, 0, sizeof(cfg)); cfg.device = d.device;
    mkp_ctx* ctx = nullptr;
    if (mkp_ctx_create(&cfg, &ctx) != MKP_OK) throw Error(MKP_E_DEVICE, "no usable gfx950 device (libmkpileup has no CPU path)");
    struct OwnedCtx { mkp_ctx* c; ~OwnedCtx() { mkp_ctx_destroy(c); } } owned{ctx};
    mkp_dmr_sites_config sc; memset(&sc, 0, sizeof(sc));
    sc.contig_names = name_ptrs.data(); sc.n_contigs = (uint32_t)name_ptrs.size(); sc.bases = d.bases.data(); sc.n_bases = (uint32_t)d.bases.size();
    sc.codes = codes.data(); sc.code_bases = code_bases.data(); sc.n_lookup = (uint32_t)codes.size(); sc.respect_mask = d.mask ? 1 : 0;
    sc.min_valid_coverage = d.min_cov; sc.prior_alpha = d.prior[0]; sc.prior_beta = d.prior[1]; sc.delta = d.delta;
    sc.have_max_coverages = d.have_max ? 1 : 0; sc.max_coverages[0] = d.max_cov[0]; sc.max_coverages[1] = d.max_cov[1];
    sc.n_sample_records = d.n_sample; sc.interval_size = d.interval; sc.batch_size = d.batch_size;
    must(ctx, mkp_dmr_sites_begin(ctx, &sc));
    auto t_ref = std::chrono::steady_clock::now();
    for (size_t tid = 0; tid < names.size(); tid++) { const FastaSeq* seq = fasta.get(names[tid]);
      must(ctx, mkp_dmr_sites_set_reference(ctx, (int32_t)tid, (const uint8_t*)seq->data(), seq->size())); }
    const double ref_ms = ms_since(t_ref);
    auto t_read = std::chrono::steady_clock::now();
    const bool host_read = Knobs::one("MKP_HOST_BEDMETHYL");
    for (int sample = 0; sample < 2; sample++) {
      const std::string& path = sample ? d.b[0] : d.a[0];
      if (!host_read) { must(ctx, mkp_dmr_sites_add_file(ctx, sample, path.c_str(), nullptr)); continue; }
      const mkp_bedmethyl_file f = read_bedmethyl_text(path);
      for (size_t k = 0; k < f.runs.size(); k++) {
        const auto it = std::find(names.begin(), names.end(), f.runs[k].chrom);
        if (it == names.end()) continue;
        const mkp_rows rows = f.rows_of(k);
        must(ctx, mkp_dmr_sites_add_rows(ctx, sample, (int32_t)(it - names.begin()), &rows));
      }
    }
    const double read_ms = ms_since(t_read);
    auto t_get = std::chrono::steady_clock::now();
    mkp_dmr_sites_out t; must(ctx, mkp_dmr_sites_get(ctx, &t));
    const double get_ms = ms_since(t_get);
    auto t_out = std::chrono::steady_clock::now();
    const std::string text = dmr_sites_table_text(t, name_ptrs.data(), d.header);
    if (to_stdout) { if (fwrite(text.data(), 1, text.size(), stdout) != text.size()) throw Error(MKP_E_IO, "short write on stdout"); fflush(stdout); }
    else write_text_file(d.out, text);
    if (n_written) *n_written = t.n_sites;
    if (d.stats) { double ms[7] = {0, 0, 0, 0, 0, 0, 0}; mkp_internal_dmr_sites_timing(ctx, ms);
      fprintf(stderr, "[mkpileup] dmr sites: written=%llu model_failures=%llu batches=%llu dropped=%llu max_coverages=%u,%u sampled=%llu,%llu; reader=%s fasta_ms=%.1f reference_upload_ms=%.1f read_ms=%.1f get_ms=%.1f (listed %.3f, heads %.3f, estimate %.3f, bad+join %.3f, score %.3f, read-back %.3f, assembly %.3f) text_ms=%.1f total_ms=%.1f\n",
          (unsigned long long)t.n_sites, (unsigned long long)t.n_model_failures, (unsigned long long)t.n_batches, (unsigned long long)t.n_batches_dropped,
          t.max_coverages[0], t.max_coverages[1], (unsigned long long)t.n_sampled[0], (unsigned long long)t.n_sampled[1], host_read ? "host" : "device",
          load_ms, ref_ms, read_ms, get_ms, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6], ms_since(t_out), ms_since(t_all)); }
    return MKP_OK;
  });
}

// ---- `mkpileup dmr replicates` = `modkit dmr pair` without -r over several -a / -b tables, in the stages of mkp_dmr_sites_main.  A command of
// its own because `dmr sites` with a second -a or -b is refused, and the suite pins that refusal.
extern "C" int mkp_host_dmr_reps_balance(const uint64_t* n_mod, const uint32_t* has_code, const uint64_t* total, uint32_t n_samples, uint32_t n_codes,
    uint64_t* out_mod, uint32_t* out_has, uint64_t* out_total, int* failed) {
  if (!has_code || !total || !out_has || !out_total || !failed || !n_samples || n_codes > MKP_DMR_SITE_MAX_CODES) return MKP_E_INVALID;
  if ((!n_mod || !out_mod) && n_codes) return MKP_E_INVALID;
  *failed = dmr_reps_balance<uint64_t>(n_mod, has_code, total, n_samples, n_codes, out_mod, out_has, out_total) ? 0 : 1;
  return MKP_OK;
}
extern "C" uint32_t mkp_host_dmr_reps_pct(uint32_t n_present, uint32_t n_samples) { return dmr_reps_pct_samples(n_present, n_samples); }

namespace {
std::string dmr_reps_table_text(const mkp_dmr_reps_out& t, const char* const* contig_names, bool header) {
  const uint64_t n = t.sites.n_sites, piece = 8192, np = (n + piece - 1) / piece;
  std::vector<std::string> parts((size_t)np);
  HostPool::get().parallel((size_t)np, [&](size_t i) { dmr_reps_rows_text(parts[i], t, contig_names, i * piece, std::min<uint64_t>(n, (i + 1) * piece),
      f32_display); });
  size_t total = 0; for (const std::string& p : parts) total += p.size();
  std::string s; s.reserve(total + 512);
  if (header) s = dmr_reps_header(dmr_reps_multiple(t), dmr_reps_matched(t));
  for (const std::string& p : parts) s += p;
  return s;
}
}  // namespace

extern "C" int mkp_host_dmr_reps_table(const mkp_dmr_reps_out* sites, const char* const* contig_names, uint32_t n_contigs, int with_header,
    const char* out_path) {
  if (!sites || !out_path || (!contig_names && n_contigs)) return MKP_E_INVALID;
  if (!sites->n_a || !sites->n_b) return MKP_E_INVALID;
  return guarded_status([&]() {
    const mkp_dmr_sites_out& T = sites->sites;
    for (uint64_t i = 0; i < T.n_sites; i++) {
      if (T.tid[i] < 0 || (uint32_t)T.tid[i] >= n_contigs) throw Error(MKP_E_INVALID, "site " + std::to_string(i) + " lies on a contig without a name");
      if (dmr_reps_matched(*sites) && sites->n_rep[i] > sites->n_a) throw Error(MKP_E_INVALID, "site " + std::to_string(i) + " lists more replicate pairs than samples");
    }
    write_text_file(out_path, dmr_reps_table_text(*sites, contig_names, with_header != 0)); return MKP_OK; });
}

extern "C" int mkp_dmr_reps_main(int argc, const char* const* argv, uint64_t* n_written, char* errbuf, size_t errbuf_len) {
  if (n_written) *n_written = 0;
  return guarded_buf(errbuf, errbuf_len, [&]() {
    const DmrSitesArgs d = parse_dmr_sites_args(argc, argv, true);
    std::vector<uint32_t> codes; std::vector<uint8_t> code_bases;
    { DmrArgs lookup_args; lookup_args.assign = d.assign; dmr_code_lookup(lookup_args, &codes, &code_bases); }
    const bool to_stdout = d.out.empty() || d.out == "-" || d.out == "stdout";
    struct stat sb;
    if (!to_stdout && !d.force && stat(d.out.c_str(), &sb) == 0) throw Error(MKP_E_IO, "refusing to overwrite existing file " + d.out);
    auto t_all = std::chrono::steady_clock::now();
    const Fasta fasta = Fasta::load(d.ref);
    const double load_ms = ms_since(t_all);
    std::vector<std::string> names; std::vector<const char*> name_ptrs;
    for (const auto& kv : fasta.seqs) names.push_back(kv.first);
    for (const std::string& s : names) name_ptrs.push_back(s.c_str());
    mkp_config cfg; memset(&cfg, 0, sizeof(cfg)); cfg.device = d.device;
    mkp_ctx* ctx = nullptr;
    if (mkp_ctx_create(&cfg, &ctx) != MKP_OK) throw Error(MKP_E_DEVICE, "no usable gfx950 device (libmkpileup has no CPU path)");
    struct OwnedCtx { mkp_ctx* c; ~OwnedCtx() { mkp_ctx_destroy(c); } } owned{ctx};
    mkp_dmr_sites_config sc; memset(&sc, 0, sizeof(sc));
    sc.contig_names = name_ptrs.data(); sc.n_contigs = (uint32_t)name_ptrs.size(); sc.bases = d.bases.data(); sc.n_bases = (uint32_t)d.bases.size();
    sc.codes = codes.data(); sc.code_bases = code_bases.data(); sc.n_lookup = (uint32_t)codes.size(); sc.respect_mask = d.mask ? 1 : 0;
    sc.min_valid_coverage = d.min_cov; sc.prior_alpha = d.prior[0]; sc.prior_beta = d.prior[1]; sc.delta = d.delta;
    sc.have_max_coverages = d.have_max ? 1 : 0; sc.max_coverages[0] = d.max_cov[0]; sc.max_coverages[1] = d.max_cov[1];
    sc.n_sample_records = d.n_sample; sc.interval_size = d.interval; sc.batch_size = d.batch_size;
    must(ctx, mkp_dmr_reps_begin(ctx, &sc, (uint32_t)d.a.size(), (uint32_t)d.b.size(), d.cap ? 1 : 0));
    auto t_ref = std::chrono::steady_clock::now();
    for (size_t tid = 0; tid < names.size(); tid++) { const FastaSeq* seq = fasta.get(names[tid]);
      must(ctx, mkp_dmr_reps_set_reference(ctx, (int32_t)tid, (const uint8_t*)seq->data(), seq->size())); }
    const double ref_ms = ms_since(t_ref);
    auto t_read = std::chrono::steady_clock::now();
    const bool host_read = Knobs::one("MKP_HOST_BEDMETHYL");
    for (int side = 0; side < 2; side++) for (size_t rep = 0; rep < (side ? d.b : d.a).size(); rep++) {
      const std::string& path = (side ? d.b : d.a)[rep];
      if (!host_read) { must(ctx, mkp_dmr_reps_add_file(ctx, side, (int)rep, path.c_str(), nullptr)); continue; }
      const mkp_bedmethyl_file f = read_bedmethyl_text(path);
      for (size_t k = 0; k < f.runs.size(); k++) {
        const auto it = std::find(names.begin(), names.end(), f.runs[k].chrom);
        if (it == names.end()) continue;
        const mkp_rows rows = f.rows_of(k);
        must(ctx, mkp_dmr_reps_add_rows(ctx, side, (int)rep, (int32_t)(it - names.begin()), &rows));
      }
    }
    const double read_ms = ms_since(t_read);
    auto t_get = std::chrono::steady_clock::now();
    mkp_dmr_reps_out t; must(ctx, mkp_dmr_reps_get(ctx, &t));
    const double get_ms = ms_since(t_get);
    auto t_out = std::chrono::steady_clock::now();
    const std::string text = dmr_reps_table_text(t, name_ptrs.data(), d.header);
    if (to_stdout) { if (fwrite(text.data(), 1, text.size(), stdout) != text.size()) throw Error(MKP_E_IO, "short write on stdout"); fflush(stdout); }
    else write_text_file(d.out, text);
    if (n_written) *n_written = t.sites.n_sites;
    if (d.stats) { double ms[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; mkp_internal_dmr_reps_timing(ctx, ms);
      fprintf(stderr, "[mkpileup] dmr replicates: a=%u b=%u written=%llu model_failures=%llu batches=%llu dropped=%llu max_coverages=%u,%u sampled=%llu,%llu; reader=%s fasta_ms=%.1f reference_upload_ms=%.1f read_ms=%.1f get_ms=%.1f (listed %.3f, heads %.3f, estimate %.3f, bad+join %.3f, gather %.3f, tasks %.3f, score %.3f, read-back %.3f, assembly %.3f) text_ms=%.1f total_ms=%.1f\n",
          t.n_a, t.n_b, (unsigned long long)t.sites.n_sites, (unsigned long long)t.sites.n_model_failures, (unsigned long long)t.sites.n_batches,
          (unsigned long long)t.sites.n_batches_dropped, t.sites.max_coverages[0], t.sites.max_coverages[1], (unsigned long long)t.sites.n_sampled[0],
          (unsigned long long)t.sites.n_sampled[1], host_read ? "host" : "device", load_ms, ref_ms, read_ms, get_ms, ms[0], ms[1], ms[2], ms[3], ms[4],
          ms[5], ms[6], ms[7], ms[8], ms_since(t_out), ms_since(t_all)); }
    return MKP_OK;
  });
}

extern "C" int mkp_pileup_main(int argc, const char* const* argv, char* errbuf, size_t errbuf_len) {
  return guarded_buf(errbuf, errbuf_len, [&]() { Args a; parse_args(argc, argv, &a, true); return run(a, nullptr, nullptr); });
}

extern "C" int mkp_pileup_hemi_main(int argc, const char* const* argv, char* errbuf, size_t errbuf_len) {
  return guarded_buf(errbuf, errbuf_len, [&]() { Args a; parse_args(argc, argv, &a, true, true); return run(a, nullptr, nullptr); });
}

extern "C" int mkp_pileup_hemi_run(mkp_ctx* ctx, int argc, const char* const* argv, mkp_run_report* report) {
  if (!ctx) return MKP_E_INVALID;
  return guarded_ctx(ctx, [&]() { Args a; parse_args(argc, argv, &a, true, true); return run(a, ctx, report); });
}

// The same subcommand on a context the caller owns: the last shard stays resident in HBM afterwards (mkp_shard_rerun
// re-launches the kernels on it) and the per-stage wall times come back in `report`.
extern "C" int mkp_pileup_run(mkp_ctx* ctx, int argc, const char* const* argv, mkp_run_report* report) {
  if (!ctx) return MKP_E_INVALID;
  return guarded_ctx(ctx, [&]() {
    Args a; parse_args(argc, argv, &a, true);
    if (a.plan_only) throw Error(MKP_E_INVALID, "--plan-only needs no context: use mkp_pileup_main");
    return run(a, ctx, report);
  });
}

extern "C" int mkp_pileup_run_cb(mkp_ctx* ctx, int argc, const char* const* argv, mkp_threshold_fn fn, void* user, mkp_run_report* report) {
  if (!ctx) return MKP_E_INVALID;
  return guarded_ctx(ctx, [&]() {
    Args a; parse_args(argc, argv, &a, true);
    if (a.plan_only) throw Error(MKP_E_INVALID, "--plan-only needs no context: use mkp_pileup_main");
    a.thr_cb = fn; a.thr_cb_user = user;
    return run(a, ctx, report);
  });
}

namespace {
// the sampling half of get_threshold_from_options: parse the sampling flags, set the caller's collapse / edge filter, walk the schedule
void sample_bam(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv, float* q_out, const mkp_caller* thresholds = nullptr,
    bool serial_without_index = false /* sample-probs / summary / extract calls: the reference's own choice (reads_sampler/mod.rs:47) */) {
  Args a; parse_args(argc, argv, &a, false); a.in_bam = bam_path;
  std::unique_ptr<BamSource> src = BamSource::open(a.in_bam,
      std::max(std::max<unsigned>((unsigned)a.threads, 1u), std::min(32u, HostPool::host_cpus())),
      !a.no_index);   // inflate threads: --threads only steers the sampling schedule
  const BamSource& bam = *src;
  RegionSpec region, sregion; const bool hr = !a.region.empty(), hs = !a.sample_region.empty();
  if (hr) region = parse_region(a.region, bam);
  if (hs) sregion = parse_region(a.sample_region, bam);
  if (!(a.filter_percentile >= 0.0f) || a.filter_percentile > 1.0f) throw Error(MKP_E_INVALID, "filter percentile must be in [0, 1]");
  mkp_caller kc; memset(&kc, 0, sizeof(kc)); kc.max_depth = a.max_depth;
  parse_edge_filter(a, &kc);
  if (a.preset == "traditional") { kc.numeric_mode = 2; kc.collapse_code = 'h'; }
  else if (!a.ignore.empty()) { uint32_t code; if (!parse_code(a.ignore, &code)) throw Error(MKP_E_INVALID, "failed to parse mod code " + a.ignore);
    kc.numeric_mode = 2;
      kc.collapse_code = code; }
  std::vector<Contig> records = targets(bam, hr ? &region : nullptr);
  BedFilter bed_store; const BedFilter* bf = nullptr;
  if (!a.include_bed.empty()) { std::map<std::string, uint32_t> c2t; for (auto& r : records) c2t[r.name] = r.tid;
    bed_store = BedFilter::load(a.include_bed, c2t);
      bf = &bed_store; }
  if (thresholds) { kc.default_threshold = thresholds->default_threshold; kc.per_mod = thresholds->per_mod; kc.n_per_mod = thresholds->n_per_mod;
                    for (int b = 0; b < 4; b++) { kc.per_base_threshold[b] = thresholds->per_base_threshold[b];
                      kc.has_per_base[b] = thresholds->has_per_base[b]; } }
  must(ctx, mkp_set_caller(ctx, &kc));
  a.serial_sampler = serial_without_index && a.world <= 1 && !bam_index_file_exists(a.in_bam);
  sample_probabilities(ctx, bam, a, hs ? &sregion : (hr ? &region : nullptr), bf);
  if (q_out) *q_out = a.filter_percentile;
}

// The pass thresholds of `summary` and `extract calls` into the caller config: explicit --filter-threshold, else --no-filtering
// (MultipleThresholdModCaller::new_passthrough: nothing is set), else the estimate from the sample that `argv`'s sampling flags describe.
// `per_mod` must outlive `k`.
void pass_thresholds(mkp_ctx* ctx, const Args& a, const char* bam_path, int argc, const char* const* argv,
    const std::vector<mkp_mod_threshold>& per_mod, mkp_caller* k) {
  if (!a.filter_threshold.empty()) parse_base_thresholds(a.filter_threshold, k);
  else if (a.no_filtering) return;
  else {
    must(ctx, mkp_histogram_begin(ctx));
    float q = 0.1f; sample_bam(ctx, bam_path, argc, argv, &q, nullptr, true);
    float thr[4]; uint8_t has[4]; thresholds_from_sample(ctx, q, thr, has, false);
    for (int b = 0; b < 4; b++) if (has[b]) { k->has_per_base[b] = 1; k->per_base_threshold[b] = thr[b]; }
  }
  k->per_mod = per_mod.data(); k->n_per_mod = (uint32_t)per_mod.size();
}

// The sampling subcommands' (`sample-probs`, `summary`) own flag names into the sampling flags of `modkit pileup`.  `own(flag)`: the
// subcommand's exceptions — true where it has dealt with the flag (or throws).
template <class Own> std::vector<std::string> sampling_subcommand_flags(int argc, const char* const* argv, Own own) {
  std::vector<std::string> tr; bool only_mapped = false, have_i = false;
  for (int i = 0; i < argc; i++) {
    const std::string s = argv[i];
    if (s == "-i" || s == "--interval-size") { tr.push_back("--sampling-interval-size"); have_i = true; }
    else if (s == "--no-sampling") { tr.push_back("-f"); tr.push_back("1.0"); }
    else if (s == "--only-mapped") only_mapped = true;
    else if (s == "--include-bed" || s == "--include-positions") { only_mapped = true; tr.push_back(s); }
    else if (own(s)) {}
    else tr.push_back(s);
  }
  if (!have_i) { tr.push_back("--sampling-interval-size"); tr.push_back("1000000"); }
  if (!only_mapped) tr.push_back("--include-unmapped");
  return tr;
}
std::vector<const char*> c_strs(const std::vector<std::string>& v) { std::vector<const char*> out; for (auto& x : v) out.push_back(x.c_str()); return out; }
}  // namespace

// get_threshold_from_options (command_utils.rs:74-134) as a call: per-base pass thresholds from the
// reference's sampling schedule; argv takes the sampling flags of `modkit pileup`
// (-n -f -p -t --sampling-interval-size --region --sample-region --include-bed --include-unmapped --edge-filter --ignore --preset).
extern "C" int mkp_estimate_thresholds(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv, float thr[4], uint8_t has[4]) {
  if (!ctx || !bam_path || !thr || !has) return MKP_E_INVALID;
  return guarded_ctx(ctx, [&]() {
    int rc = mkp_histogram_begin(ctx); if (rc != MKP_OK) return rc;
    float q = 0.1f; sample_bam(ctx, bam_path, argc, argv, &q);
    thresholds_from_sample(ctx, q, thr, has, false);
    return (int)MKP_OK;
  });
}

// `modkit sample-probs` (SampleModBaseProbs::run, src/commands.rs:680-887), the percentiles table: the schedule's sample, per canonical
// base the requested percentiles of the argmax probabilities (Percentiles::new -> percentile_linear_interp).  The subcommand's own
// flag names: -i is the sampling interval (default 1 000 000), unmapped reads are sampled unless --only-mapped (or --include-bed).
extern "C" int mkp_sample_probs(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv, const float* percentiles,
    uint32_t n_percentiles,
                                float* values /* [4][n_percentiles], bases A,C,G,T */, uint8_t has[4], uint64_t n_values[4]) {
  if (!ctx || !bam_path || (!percentiles && n_percentiles) || !values || !has || !n_values) return MKP_E_INVALID;
  return guarded_ctx(ctx, [&]() {
    const std::vector<std::string> tr = sampling_subcommand_flags(argc, argv, [](const std::string& s) -> bool {
      if (s == "-p" || s == "--percentiles" || s == "--filter-percentile") throw Error(MKP_E_INVALID,
          "percentiles are an argument of this call, not a flag");
      return false; });
    const std::vector<const char*> av = c_strs(tr);
    int rc = mkp_histogram_begin(ctx); if (rc != MKP_OK) return rc;
    sample_bam(ctx, bam_path, (int)av.size(), av.data(), nullptr, nullptr, true);
    for (int b = 0; b < 4; b++) { has[b] = 0; n_values[b] = 0; }
    for (uint32_t k = 0; k < n_percentiles; k++) {
      const float q = percentiles[k];
      if (!(q >= 0.0f) || q > 1.0f) throw Error(MKP_E_INVALID, "percentiles must be in [0, 1]");
      float thr[4]; uint8_t h[4]; uint64_t n[4] = {0, 0, 0, 0};
      thresholds_from_sample(ctx, q, thr, h, false, n);
      for (int b = 0; b < 4; b++) { values[(size_t)b * n_percentiles + k] = thr[b]; has[b] = h[b]; n_values[b] = n[b]; }
    }
    if (n_percentiles == 0) { float thr[4]; uint64_t n[4] = {0, 0, 0, 0}; try { thresholds_from_sample(ctx, 0.5f, thr, has, false, n);
        } catch (const Error&) {} for (int b = 0; b < 4; b++) n_values[b] = n[b]; }
    return (int)MKP_OK;
  });
}

// `modkit summary` (ModSummarize::run, src/commands.rs:1035-1189): ModSummary as counts.  Two walks of the same sampling schedule on the
// device: the first estimates the pass thresholds (calc_thresholds_per_base) unless the flags give them, the second counts every sampled
// call under its thresholded call, or under its argmax call when that is Filtered (sampled_reads_to_summary, src/summarize.rs:117-262).
extern "C" int mkp_summary(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv, mkp_summary_out* out) {
  if (!ctx || !bam_path || !out) return MKP_E_INVALID;
  struct ModeGuard { mkp_ctx* c; ~ModeGuard() { c->summary_mode = false; } } guard{ctx};
  return guarded_ctx(ctx, [&]() {
    const std::vector<std::string> tr = sampling_subcommand_flags(argc, argv, [](const std::string& s) { return s == "--tsv" || s == "--table"; });
    const std::vector<const char*> av = c_strs(tr);
    Args a; parse_args((int)av.size(), av.data(), &a, false);
    mkp_caller kt; memset(&kt, 0, sizeof(kt));
    const std::vector<mkp_mod_threshold> per_mod = parse_mod_thresholds(a.mod_thresholds);
    pass_thresholds(ctx, a, bam_path, (int)av.size(), av.data(), per_mod, &kt);
    ctx->summary_mode = true;
    int rc = mkp_internal_summary_begin(ctx); if (rc != MKP_OK) return rc;
    sample_bam(ctx, bam_path, (int)av.size(), av.data(), nullptr, &kt, true);
    uint64_t t[134]; std::vector<MkpSlot> slots;
    rc = mkp_internal_summary_get(ctx, t, &slots); if (rc != MKP_OK) return rc;
    ctx->h_sum_base.clear(); ctx->h_sum_code.clear(); ctx->h_sum_pass.clear(); ctx->h_sum_fail.clear();
    const uint64_t obs = t[128 + 5];
    for (uint32_t b = 0; b < 4; b++) {
      out->reads_with_mod_calls[b] = t[128 + b]; out->threshold[b] = kt.per_base_threshold[b]; out->has_threshold[b] = kt.has_per_base[b];
      if (!t[128 + b]) continue;
      auto row = [&](uint32_t code, uint32_t cls) { ctx->h_sum_base.push_back((uint8_t)b); ctx->h_sum_code.push_back(code);
        ctx->h_sum_pass.push_back(t[b * 32 + cls]);
          ctx->h_sum_fail.push_back(t[b * 32 + 16 + cls]); };
      row(MKP_HEMI_CANONICAL, 1);
      std::vector<std::pair<uint32_t, uint32_t>> codes;
      for (size_t si = 0; si < slots.size() && si < 14; si++) if (slots[si].pb == b
          && ((obs >> si) & 1ull)) codes.push_back({slots[si].code_repr, (uint32_t)si});
      std::sort(codes.begin(), codes.end());
      for (auto& cs : codes) row(cs.first, 2 + cs.second);
    }
    out->total_reads_used = t[128 + 4];
    out->n_rows = (uint32_t)ctx->h_sum_base.size(); out->base = ctx->h_sum_base.data(); out->code_repr = ctx->h_sum_code.data();
      out->pass_count = ctx->h_sum_pass.data();
        out->fail_count = ctx->h_sum_fail.data();
    return (int)MKP_OK;
  });
}

// The sampling half alone, for multi-GPU runs: add this rank's share of the sample (argv carries --gpus-rank R --gpus-world W
// next to the sampling flags; W > 1 needs -f 1.0) to the context's histograms.  The caller then sums mkp_histogram_get's arrays
// over the ranks (RCCL all-reduce) and finishes with mkp_histogram_locate / _resolve / mkp_percentile_from_histogram.
extern "C" int mkp_histogram_add_bam(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv) {
  if (!ctx || !bam_path) return MKP_E_INVALID;
  return guarded_ctx(ctx, [&]() { sample_bam(ctx, bam_path, argc, argv, nullptr); return MKP_OK; });
}

// process_region_batch stand-in reading the BAM itself: an indexed BAM goes through the device ingest (compressed blocks up, records cut and
// packed in HBM — what mkp_pileup_run does per shard), anything else through the host reader + packer
extern "C" int mkp_process_region(mkp_ctx* ctx, const char* bam_path, const mkp_shard* shard, mkp_rows* out) {
  if (!ctx || !bam_path || !shard || !out) return MKP_E_INVALID;
  return guarded_ctx(ctx, [&]() {
    std::unique_ptr<BamSource> src = BamSource::open(bam_path, 0);
    if (src->indexed() && ctx->partition_tags.empty() && !Knobs().host_ingest && shard->tid >= 0 && shard->end > shard->start) {
      if (!ctx->ingest) { ctx->ingest = mkp_internal_ingest_create(ctx->device);
        if (!ctx->ingest) throw Error(MKP_E_DEVICE, "device ingest: cannot create streams on the device");
        }
      std::unique_ptr<DevShard> dev = mkp_internal_ingest_run(ctx->ingest, *src, (uint32_t)shard->tid,
          shard->start > MKP_HALO ? (uint32_t)shard->start - MKP_HALO : 0u, (uint32_t)shard->end + MKP_HALO);
      int rc = mkp_shard_begin(ctx, shard); if (rc != MKP_OK) return rc;
      rc = mkp_internal_shard_attach(ctx, dev.get()); mkp_internal_ingest_recycle(ctx->ingest, dev.get()); if (rc != MKP_OK) return rc;
      return mkp_shard_run(ctx, out);
    }
    int rc = mkp_shard_begin(ctx, shard); if (rc != MKP_OK) return rc;
    BamBatch batch; src->fetch((uint32_t)shard->tid, shard->start > MKP_HALO ? shard->start - MKP_HALO : 0, shard->end + MKP_HALO, &batch);
    std::vector<mkp_record> recs; for (auto& e : batch.recs) recs.push_back(batch.view(e));
    rc = mkp_shard_add_records(ctx, recs.data(), (uint32_t)recs.size()); if (rc != MKP_OK) return rc;
    return mkp_shard_run(ctx, out);
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// `modkit extract calls` (EntryExtractCalls::run, src/extract/subcommand.rs:452-761): the per-read call table.  The reads are decoded
// on the device by the sampling kernels in per-call mode (MM / ML -> BaseModProbs, edge filter, ReDistribute collapse, the argmax call
// and the thresholded call — mkp_kernels.hip, sample_mode 3); what is left for the host is what the table is made of besides the
// call: read ids, soft clips, reference positions (aligned_pairs_full), base qualities, k-mers, and the text
// (PositionModCalls::to_row, src/extract/writer.rs:46-132).  Records are taken in FILE order — the reference's serial path
// (process_records_to_chan, src/extract/util.rs:519-575), which its golden tests pin; its indexed path hands interval batches to the
// writer in whatever order the Rayon pool finishes them.
namespace {
// f32 through Rust's Display: the shortest decimal that parses back to the same f32, positional notation
std::string f32_display(float v) {
  if (v == 0.0f) return std::signbit(v) ? "-0" : "0";
  char buf[64]; int prec = 1;
  for (; prec <= 9; prec++) { snprintf(buf, sizeof(buf), "%.*e", prec - 1, (double)v); if (strtof(buf, nullptr) == v) break; }
  std::string s(buf); const size_t e = s.find('e'); const int ex = atoi(s.c_str() + e + 1);
  std::string mant = s.substr(0, e); bool neg = false;
  if (!mant.empty() && mant[0] == '-') { neg = true; mant.erase(0, 1); }
  std::string digits; for (char c : mant) if (c != '.') digits.push_back(c);
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  std::string out;
  if (ex >= 0) { if ((int)digits.size() <= ex + 1) out = digits + std::string((size_t)(ex + 1 - (int)digits.size()), '0');
    else out = digits.substr(0, (size_t)ex + 1) + "." + digits.substr((size_t)ex + 1);
    }
  else out = "0." + std::string((size_t)(-ex - 1), '0') + digits;
  return neg ? "-" + out : out;
}
char comp_char(char c) {   // bio::alphabets::dna::revcomp
  switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'N': return 'N';
    case 'R': return 'Y'; case 'Y': return 'R'; case 'K': return 'M'; case 'M': return 'K'; case 'B': return 'V'; case 'V': return 'B';
      case 'D': return 'H'; case 'H': return 'D';
    default: return c;
  }
}
// Kmer::new (util.rs:750-777) as text; '-' where the sequence has no base
std::string kmer_at(const char* seq, size_t n, size_t position, size_t size) {
  const size_t before = size % 2 == 0 ? size / 2 - 1 : size / 2, after = size / 2;
  std::string k;
  for (size_t off = before; off >= 1; off--) k.push_back(position >= off && position - off < n ? seq[position - off] : '-');
  k.push_back(position < n ? seq[position] : '-');
  for (size_t off = 1; off <= after; off++) k.push_back(position + off < n ? seq[position + off] : '-');
  return k;
}

// ---- the stages of mkp_extract_calls_main

// the subcommand's own flags; `rest`: everything else — the flags of the threshold estimate and the two positionals (parse_args)
struct ExtractFlags {
  std::string ref_path, exclude_bed; std::vector<std::string> motif_parts, rest; bool cpg = false, bgzf = false;
  bool allow_np = false, mapped_only = false, pass_only = false, no_headers = false, stats = false, ignore_index = false, ignore_implicit = false;
  size_t kmer = 5; int device = 0; long num_reads = -1;
};
ExtractFlags parse_extract_flags(int argc, const char* const* argv) {
  ExtractFlags f;
  for (int i = 0; i < argc; i++) {
    const std::string s = argv[i];
    auto val = [&]() { if (i + 1 >= argc) throw Error(MKP_E_INVALID, "missing value for " + s); return std::string(argv[++i]); };
    if (s == "--ref" || s == "--reference") f.ref_path = val(); else if (s == "--allow-non-primary") f.allow_np = true;
      else if (s == "--mapped-only") f.mapped_only = true;
    else if (s == "--pass-only" || s == "--pass") f.pass_only = true; else if (s == "--no-headers") f.no_headers = true;
      else if (s == "--kmer-size") f.kmer = std::stoul(val());
    else if (s == "--force" || s == "--suppress-progress") {} else if (s == "--device") f.device = std::stoi(val());
      else if (s == "--stats") f.stats = true;
    else if (s == "--num-reads") f.num_reads = std::stol(val()); else if (s == "--ignore-index") f.ignore_index = true;
    else if (s == "--ignore-implicit") f.ignore_implicit = true;
    else if (s == "--exclude-bed" || s == "-v" || s == "--exclude-positions") f.exclude_bed = val();
    else if (s == "--motif") { f.motif_parts.push_back(val()); f.motif_parts.push_back(val()); } else if (s == "--cpg") f.cpg = true;
    else if (s == "--bgzf") f.bgzf = true; else if (s == "--out-threads") val();
    else f.rest.push_back(s);
  }
  if (f.kmer == 0 || f.kmer > 50) throw Error(MKP_E_INVALID, "kmer size must be less than or equal to 50");
  if (f.pass_only && std::find(f.rest.begin(), f.rest.end(), "--no-filtering") != f.rest.end()) throw Error(MKP_E_INVALID,
      "the argument '--no-filtering' cannot be used with '--pass-only'");
  return f;
}

BedFilter load_bed_for(const std::string& path, const BamData& bd) {
  std::map<std::string, uint32_t> c2t; for (size_t t = 0; t < bd.ref_names.size(); t++) c2t[bd.ref_names[t]] = (uint32_t)t;
  return BedFilter::load(path, c2t);
}
struct TempFile { std::string path; ~TempFile() { if (!path.empty()) unlink(path.c_str()); } };   // unlinked on every exit path
// --motif / --cpg (load_regions, src/extract/util.rs:157-277): the include filter becomes the motif hits over every contig of the FASTA that
// the header names — the whole sequence, lower case matching unless --mask — one position per hit and strand, intersected with the
// --include-bed positions (`bed`) when both are given.  From there on it IS the include filter: rows, the estimate (handed over as a BED
// file of its own, `tmp`), the schedule.
BedFilter motif_include_filter(const ExtractFlags& f, bool mask, const BamData& bd, const Fasta& fasta, const BedFilter* bed, TempFile* tmp) {
  if (f.ref_path.empty()) throw Error(MKP_E_INVALID, "--motif / --cpg need --ref");
  std::vector<std::string> parts = f.motif_parts;   // RegexMotif::from_raw_parts (motif_bed.rs:152-195)
  if (f.cpg) { bool has = false; for (size_t i = 0; i + 1 < parts.size(); i += 2) if (parts[i] == "CG" && parts[i + 1] == "0") has = true;
    if (!has) { parts.push_back("CG"); parts.push_back("0"); } }
  std::vector<Motif> motifs;
  for (size_t i = 0; i + 1 < parts.size(); i += 2) motifs.push_back(Motif::parse(parts[i], std::stoul(parts[i + 1])));
  BedFilter mf;
  for (size_t t = 0; t < bd.ref_names.size(); t++) {
    const FastaSeq* sq = fasta.get(bd.ref_names[t]); if (!sq) continue;
    std::map<uint32_t, Rule> hits;
    for (auto& m : motifs) motif_hits(sq->data(), sq->size(), m, 0, (uint32_t)t, bed, &hits, !mask);
    auto& P = mf.pos[(uint32_t)t]; auto& N = mf.neg[(uint32_t)t];   // (a searched contig is in the filter even without a hit)
    for (auto& kv : hits) { if (kv.second & R_POS) P.push_back({kv.first, (uint64_t)kv.first + 1});
      if (kv.second & R_NEG) N.push_back({kv.first, (uint64_t)kv.first + 1}); }
    merge_spans(P); merge_spans(N);
  }
  char tmpl[] = "/tmp/mkp_motif_bed_XXXXXX"; const int fd = mkstemp(tmpl);
  if (fd < 0) throw Error(MKP_E_IO, "cannot create a temporary BED for the motif positions");
  tmp->path = tmpl; FILE* bf_out = fdopen(fd, "w");
  for (auto* mp : {&mf.pos, &mf.neg}) for (auto& kv : *mp) for (auto& x : kv.second)
    fprintf(bf_out, "%s\t%llu\t%llu\t.\t0\t%c\n", bd.ref_names[kv.first].c_str(), (unsigned long long)x.s, (unsigned long long)x.e,
        mp == &mf.pos ? '+' : '-');
  fclose(bf_out);
  return mf;
}

// the flags of the threshold estimate (get_threshold_from_options, command_utils.rs:74-134): calls without a reference position count
// unless --mapped-only (ReferencePositionFilter::only_mapped_positions, src/extract/util.rs:39-41)
std::vector<std::string> extract_estimate_flags(const ExtractFlags& f, const Args& a, const std::string& motif_bed_path, bool have_bed) {
  std::vector<std::string> sf;
  for (size_t i = 0; i < f.rest.size(); i++) {
    if (f.rest[i] == a.in_bam || f.rest[i] == a.out_bed) continue;
    // (the motif positions already hold the intersection with the BED: the estimate gets them as its only --include-bed)
    if (!motif_bed_path.empty() && (f.rest[i] == "--include-bed" || f.rest[i] == "--include-positions")) { i++; continue; }
    sf.push_back(f.rest[i]);
  }
  if (!motif_bed_path.empty()) { sf.push_back("--include-bed"); sf.push_back(motif_bed_path); }
  // (--include-bed: "specifying include-only BED outputs only mapped sites", util.rs:136-142 — positions without a reference position do not count)
  if (!f.mapped_only && !have_bed) sf.push_back("--include-unmapped");
  return sf;
}

// What is decided before the first record: --include-bed (ReferencePositionFilter::keep, src/extract/util.rs:44-69), --region, --num-reads
// (src/extract/util.rs:126-160, 329-575).  With an index (and without --ignore-index) the reference walks interval chunks of the targets:
// --region then selects the records its fetches return — every record overlapping the region, once — where the serial scan looks at every
// record of the file.  The reference's rows leave in the order its pool finishes the intervals; here in file order.  --num-reads: the
// serial path's "first N records that reach process_record"; on an indexed BAM it follows the sampling schedule (iv_quota).
struct ExtractPlan {
  bool use_index = false, scheduled = false, remove_inferred = false, have_region = false, include_unmapped_reads = false;
  int64_t reg_tid = -1, reg_s = 0, reg_e = 0;
  // --num-reads with an index (run_extract_reads, src/extract/util.rs:329-470; subcommand.rs:662-683): SamplingSchedule::from_num_reads over the
  // index counts; every interval of the feeder — threads * 1.5 groups of >= --interval-size bases per super batch — has a RecordSampler
  // of its own (extract_interval_quotas).  An interval's records are the ones its fetch returns that do not start in front of the previous
  // interval's end — in a sorted file: the records that start inside it (the first interval of a region also takes the records reaching
  // into it) — and it takes the first that many whose process_record succeeds.  Then the records without coordinates, unless a region /
  // --mapped-only excludes them: the first (N - used) that reach process_record.  Rows leave in interval order (the reference: in pool order).
  std::map<uint32_t, std::vector<IvQuota>> iv_quota;
};
ExtractPlan plan_extract(const ExtractFlags& f, const Args& a, const BamData& bd, const BedFilter* bed) {
  ExtractPlan p;
  { FILE* probe = fopen((a.in_bam + ".bai").c_str(), "rb"); if (probe) { fclose(probe); p.use_index = !f.ignore_index; } }
  p.scheduled = p.use_index && f.num_reads >= 0;
  // --ignore-implicit: ReadBaseModProfile::remove_inferred runs in the reference's interval path only (src/extract/util.rs:413-419); its serial
  // scan (no index, --ignore-index) takes the flag and never looks at it
  p.remove_inferred = f.ignore_implicit && p.use_index;
  p.have_region = !a.region.empty();
  p.include_unmapped_reads = !p.have_region && !f.mapped_only && !bed;   // load_regions (util.rs:136-155)
  if (!p.have_region && !p.scheduled) return p;
  std::unique_ptr<BamSource> src = BamSource::open(a.in_bam, 0);
  RegionSpec rg;
  if (p.have_region) {
    rg = parse_region(a.region, *src);
    for (size_t t = 0; t < bd.ref_names.size(); t++) if (bd.ref_names[t] == rg.name) p.reg_tid = (int64_t)t;
    p.reg_s = rg.start; p.reg_e = rg.end;
  }
  if (p.scheduled) {
    const IdxStats st = idxstats(*src, p.have_region ? &rg : nullptr, bed);
    const std::map<uint32_t, Quota> quota = num_reads_quotas(st, (size_t)f.num_reads, p.include_unmapped_reads);
    const size_t batch_size = std::max<size_t>((size_t)floorf((float)a.threads * 1.5f), 1);
    // (--include-bed: every run of BED spans is a reference record of its own — optimize_reference_records, util.rs:287-296)
    std::vector<Contig> recs_t = targets(*src, p.have_region ? &rg : nullptr);
    if (bed) recs_t = bed_contigs(*bed, recs_t, a.interval_size);
    p.iv_quota = extract_interval_quotas(feeder_groups(recs_t, a.interval_size), batch_size, quota);
  }
  return p;
}

struct ExtractCounts { uint64_t n_used = 0, n_skipped = 0, n_failed = 0, n_rows = 0; };

// The records of bd.recs[r0, r1) that go to the device (TrackingModRecordIter, mod_bam.rs:53-122, + process_records_to_chan's --mapped-only),
// with their alignment ends (one past the last reference position; a record without reference span counts as one base)
void select_records(const ExtractFlags& f, const ExtractPlan& p, const BamData& bd, const BamBatch& view, size_t r0, size_t r1,
    std::vector<mkp_record>* recs, std::vector<int64_t>* ends, ExtractCounts* c) {
  recs->clear(); ends->clear();
  for (size_t i = r0; i < r1; i++) {
    const mkp_record r = view.view(bd.recs[i]); const int64_t end = bd.recs[i].end;
    // IndexedReader::fetch(tid, start, end): the records overlapping the region
    if (p.use_index && p.have_region && (r.tid != p.reg_tid || (int64_t)r.pos >= p.reg_e || end <= p.reg_s)) continue;
    if (p.scheduled && r.tid < 0) {   // the schedule's last leg: process_records_to_chan(.., only_mapped = false, allow_non_primary = false, ..)
      if (!p.include_unmapped_reads) continue;
      if (r.flag & (2048 | 256 | 1024)) { c->n_skipped++; continue; }
    } else {
      if ((r.flag & (2048 | 256 | 1024)) && !f.allow_np) { c->n_skipped++; continue; }
    }
    if (r.l_qseq <= 0) { c->n_failed++; continue; }
    if ((r.flag & 4) && f.mapped_only && !p.scheduled) { c->n_skipped++; continue; }   // (the schedule's samplers never ask about mapping)
    recs->push_back(r); ends->push_back(end);
  }
}

// get_soft_clipped (read_ids_to_base_mod_probs.rs:803-824): the soft-clipped bases at either end of an aligned record, stored order; not
// ok — process_record's own failure — when its CIGAR holds nothing else
struct Clips { size_t start = 0, end = 0; bool ok = true; };
uint32_t cigar_word(const mkp_record& r, uint32_t k) { uint32_t w; memcpy(&w, r.data + r.l_qname + 4 * (size_t)k, 4); return w; }
Clips soft_clips(const mkp_record& r) {
  Clips c; if (r.flag & 4) return c;
  uint32_t k = 0; for (; k < r.n_cigar && (cigar_word(r, k) & 15u) == 4u; k++) c.start += cigar_word(r, k) >> 4;
  if (k == r.n_cigar) { c.ok = false; return c; }
  for (k = r.n_cigar; k-- > 0 && (cigar_word(r, k) & 15u) == 4u;) c.end += cigar_word(r, k) >> 4;
  return c;
}

// --num-reads counts what reaches process_record: records whose tags parse and hold something (an unmapped record under --mapped-only
// never gets that far: dropped in select_records).  Three ways of counting: a scheduled aligned record against its interval's sampler, a
// scheduled record without coordinates against what the aligned ones left of N, any record of an unscheduled run against N.
enum class Admit { Rows /* write its rows */, Silent /* dropped, counted nowhere */, Failed, Skipped };
struct Admission {
  const ExtractFlags& f; ExtractPlan& p; size_t aligned_used = 0; long n_sent = 0; bool done = false;   // done: no record after this one
  Admit judge(const mkp_record& r, int64_t rend, const MkpReadHdr& h, const MkpReadOut& ro, const Clips& clips) {
    const Admit not_offered = (h.flags & MKP_RF_BAD) ? Admit::Failed : Admit::Skipped;
    if (p.scheduled && r.tid >= 0) {
      auto qi = p.iv_quota.find((uint32_t)r.tid); if (qi == p.iv_quota.end() || qi->second.empty()) return Admit::Silent;
      // the interval that takes the record: the first one (feeder order) whose fetch returns it and whose `cut` — the previous interval's
      // end — does not lie behind its start: the first interval that ends behind the record's start, if the record reaches it at all
      auto it = std::upper_bound(qi->second.begin(), qi->second.end(), (int64_t)r.pos,
          [](int64_t pos, const IvQuota& q) { return pos < (int64_t)q.end; });
      if (it == qi->second.end() || (int64_t)it->start >= rend) return Admit::Silent;
      IvQuota& Q = *it;
      if (Q.nr == -2) return Admit::Silent;                      // the schedule holds nothing for this contig
      if (!ro.ok) return not_offered;                            // TrackingModRecordIter never offers it
      if (Q.nr >= 0 && Q.used >= Q.nr) return Admit::Silent;     // RecordSampler::ask -> Done
      if (!clips.ok) return Admit::Failed;                       // process_record's own failure: get_soft_clipped
      Q.used++; aligned_used++;
      if (f.mapped_only && (r.flag & 4)) return Admit::Silent;   // every row of an unmapped record lacks a reference position
      return ro.n_events ? Admit::Rows : Admit::Silent;
    }
    const long n = !p.scheduled ? f.num_reads : f.num_reads > (long)aligned_used ? f.num_reads - (long)aligned_used : 0;
    // (looked at after the record went to the writer: N = 0 lets one through)
    if (ro.ok) { n_sent++; if (f.num_reads >= 0 && n_sent >= n) done = true; }
    if (!ro.ok || !ro.n_events) return not_offered;
    return clips.ok ? Admit::Rows : Admit::Failed;
  }
};

// what the rows of a record are made from besides the record
struct RowSource {
  const ExtractFlags& f; const ExtractPlan& p; const BamData& bd; const Fasta& fasta; const BedFilter* bed; const BedFilter* exbed;
  const std::vector<MkpSlot>& slots; const std::vector<MkpEvent>& ev; const std::vector<float>& vals;
};
// The rows of one admitted record (PositionModCalls::to_row, src/extract/writer.rs:46-132) appended to `text`: forward sequence, the CIGAR
// walk to reference positions, the row filters, the text; *n_rows counts them.  True when the record is used: a call of it passed the position
// filters (whether or not --ignore-implicit / --pass-only then left a row).
bool record_rows(const RowSource& X, const mkp_record& r, const MkpReadHdr& h, const MkpReadOut& ro, const Clips& clips, std::string* text,
    uint64_t* n_rows) {
  static const char NT16[] = "=ACMGRSVTWYHKDBN";
  const bool unmapped = (r.flag & 4) != 0, rev = (r.flag & 16) != 0, have_bed = X.bed != nullptr;
  const size_t L = (size_t)r.l_qseq;
  const uint8_t* sq = r.data + r.l_qname + 4 * (size_t)r.n_cigar; const uint8_t* ql = sq + (L + 1) / 2;
  const size_t clip_start = rev ? clips.end : clips.start, clip_end = rev ? clips.start : clips.end;
  auto within = [&](size_t qp) { return L >= clip_end && qp >= clip_start && qp < L - clip_end; };
  // forward sequence and qualities
  std::string fwd(L, 'N');
  for (size_t k = 0; k < L; k++) { const uint8_t b = sq[k >> 1]; const char c = NT16[(k & 1) ? (b & 15) : (b >> 4)];
    if (rev) fwd[L - 1 - k] = comp_char(c);
    else fwd[k] = c;
    }
  const bool have_chrom = !unmapped && r.tid >= 0 && (size_t)r.tid < X.bd.ref_names.size();
  const std::string chrom = have_chrom ? X.bd.ref_names[(size_t)r.tid] : std::string();
  const FastaSeq* ref_seq = have_chrom ? X.fasta.get(chrom) : nullptr;
  const bool primary_or_unmapped = r.flag == 0 || r.flag == 16 || r.flag == 4;
  const std::string qname((const char*)r.data, r.l_qname ? (size_t)r.l_qname - 1 : 0);
  // the record's calls come in stored order (ascending stored index): one CIGAR walk gives their reference positions
  struct Row { size_t f; long ref; uint32_t info; float p; };
  std::vector<Row> rows; rows.reserve(ro.n_events);
  uint32_t ck = 0; size_t q_at = 0; long r_at = r.pos;   // op ck starts at stored index q_at / reference position r_at
  for (uint32_t k = 0; k < ro.n_events; k++) {
    const MkpEvent& e = X.ev[(size_t)h.event_off + k];
    const size_t f = e.pos, q = rev ? L - 1 - f : f;
    long ref = -1;
    if (!unmapped) {
      // an event behind the walk (the kernels emit a record's events in stored order; should that ever change, start over instead of
      // underflowing)
      if (q < q_at) { ck = 0; q_at = 0; r_at = r.pos; }
      while (ck < r.n_cigar) {
        const uint32_t w = cigar_word(r, ck), op = w & 15u, len = w >> 4;
        const bool cq = op == 0 || op == 1 || op == 4 || op == 7 || op == 8, cr = op == 0 || op == 2 || op == 3 || op == 7 || op == 8;
        if (cq && q < q_at + len) { if (op == 0 || op == 7 || op == 8) ref = r_at + (long)(q - q_at); break; }
        if (cq) q_at += len;
        if (cr) r_at += len;
        ck++;
      }
    }
    rows.push_back({f, ref, e.info, X.vals[(size_t)h.event_off + k]});
  }
  if (unmapped && rev) std::reverse(rows.begin(), rows.end());   // no alignment strand: ascending forward position
  bool any = false;
  for (const Row& w : rows) {
    if ((X.f.mapped_only || have_bed) && (unmapped || w.ref < 0)) continue;   // filter_read_base_mod_probs (src/extract/util.rs:71-124)
    // ... asked with the reference strand of the mod
    if (have_bed && !X.bed->contains((uint32_t)r.tid, (uint64_t)w.ref, (((w.info >> 2) & 1u) != 0) != rev)) continue;
    // --exclude-bed (load_regions, util.rs:177-187; ReferencePositionFilter::keep = include hit && !exclude hit): a row filter only
    if (X.exbed && !unmapped && w.ref >= 0 && X.exbed->contains((uint32_t)r.tid, (uint64_t)w.ref, (((w.info >> 2) & 1u) != 0) != rev)) continue;
    if (!primary_or_unmapped && !within(w.f)) continue;                   // iter_profiles (read_ids_to_base_mod_probs.rs:785-800)
    any = true;
    const uint32_t tb = w.info & 3u, sg = (w.info >> 2) & 1u, inferred = (w.info >> 3) & 1u, thr_cls = (w.info >> 4) & 15u,
        arg_cls = (w.info >> 8) & 15u;
    if (X.p.remove_inferred && inferred) continue;
    const bool filtered = thr_cls == 0;
    if (filtered && X.f.pass_only) continue;
    std::string code = "-";
    if (arg_cls >= 2) { const uint32_t cr = arg_cls - 2 < X.slots.size() ? X.slots[arg_cls - 2].code_repr : 0u;
      code = (cr & 0x80000000u) ? std::to_string(cr & 0x7fffffffu) : std::string(1, (char)cr); }
    std::string qk = kmer_at(fwd.data(), L, w.f, X.f.kmer);
    if (sg) { std::string t; for (size_t k = qk.size(); k-- > 0;) t.push_back(qk[k] == '-' ? '-' : comp_char(qk[k])); qk.swap(t); }
    std::string rk = ".";
    if (w.ref >= 0 && ref_seq) rk = kmer_at(ref_seq->data(), ref_seq->size(), (size_t)w.ref, X.f.kmer);
    const unsigned bq = ql[rev ? L - 1 - w.f : w.f];
    char line[1200];
    const int ln = snprintf(line, sizeof(line), "%s\t%zu\t%ld\t%s\t%c\t%c\t%c\t%zu\t%zu\t%zu\t%s\t%s\t%u\t%s\t%s\t%c\t%c\t%s\t%s\t%s\t%u\n",
        qname.c_str(), w.f, w.ref >= 0 ? w.ref : -1L,
             have_chrom ? chrom.c_str() : ".", sg ? '-' : '+', unmapped ? '.' : (rev ? '-' : '+'),
                 unmapped ? '.' : ((sg != 0) != rev ? '-' : '+'), clip_start, clip_end, L,
             f32_display(w.p).c_str(), code.c_str(), bq, rk.c_str(), qk.c_str(), "ACGT"[tb], "ACGT"[sg ? 3 - tb : tb],
                 filtered ? "true" : "false", inferred ? "true" : "false",
             (have_chrom && within(w.f)) ? "true" : "false", (unsigned)r.flag);
    if (ln < 0 || (size_t)ln >= sizeof(line)) throw Error(MKP_E_UNSUPPORTED,
        "extract calls: a row is longer than " + std::to_string(sizeof(line)) + " bytes (read or contig name of unusual length)");
    text->append(line, (size_t)ln); (*n_rows)++;
  }
  return any;
}
}  // namespace

namespace {
// The table's sink: the output file (or stdout) as plain text, or — --bgzf (src/extract/subcommand.rs:629-660) — the same table as BGZF
// blocks (SAM spec 4.1) cut at 0xff00 bytes, closed by the empty EOF block
struct TableSink {
  std::string path; bool bgzf; FILE* out; std::vector<uint8_t> pend, z;
  TableSink(const std::string& p, bool bgzf_blocks) : path(p), bgzf(bgzf_blocks), out((p == "-" || p == "stdout") ? stdout : fopen(p.c_str(), "w+")) {
    if (!out) throw Error(MKP_E_IO, "failed to make output file " + path); }
  ~TableSink() { if (out && out != stdout) fclose(out); }
  void write(const void* p, size_t n) { if (n && fwrite(p, 1, n, out) != n) throw Error(MKP_E_IO, "write error on " + path); }
  void put(const char* p, size_t n) {
    if (!bgzf) { write(p, n); return; }
    pend.insert(pend.end(), (const uint8_t*)p, (const uint8_t*)p + n);
    size_t at = 0; z.clear();
    while (pend.size() - at >= MKP_BGZF_BLOCK) { bgzf_block(pend.data() + at, MKP_BGZF_BLOCK, &z); at += MKP_BGZF_BLOCK; }
    pend.erase(pend.begin(), pend.begin() + (long)at);
    write(z.data(), z.size());
  }
  void finish() {
    if (!bgzf) return;
    z.clear(); if (!pend.empty()) bgzf_block(pend.data(), pend.size(), &z);
    static const uint8_t eof_block[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    z.insert(z.end(), eof_block, eof_block + 28);
    write(z.data(), z.size());
  }
};
}  // namespace

extern "C" int mkp_extract_calls_main(int argc, const char* const* argv, char* errbuf, size_t errbuf_len) {
  mkp_ctx* ctx = nullptr;
  struct Guard { mkp_ctx** c; ~Guard() { if (*c) mkp_ctx_destroy(*c); } } guard{&ctx};
  return guarded_buf(errbuf, errbuf_len, [&]() {
    const ExtractFlags f = parse_extract_flags(argc, argv);
    const std::vector<const char*> av = c_strs(f.rest);
    Args a; parse_args((int)av.size(), av.data(), &a, true);
    const BamData bd = load_bam(a.in_bam, 0, false);
    Fasta fasta; if (!f.ref_path.empty()) fasta = Fasta::load(f.ref_path);
    // the include filter: --include-bed, or the motif positions (within the BED when both are given)
    BedFilter bed; bool have_bed = !a.include_bed.empty();
    if (have_bed) bed = load_bed_for(a.include_bed, bd);
    TempFile motif_bed;
    if (f.cpg || !f.motif_parts.empty()) { bed = motif_include_filter(f, a.mask, bd, fasta, have_bed ? &bed : nullptr, &motif_bed); have_bed = true; }
    const std::vector<std::string> sf = extract_estimate_flags(f, a, motif_bed.path, have_bed);
    const std::vector<const char*> sav = c_strs(sf);
    // the device and its caller: thresholds, edge filter, --ignore
    mkp_config cfg; memset(&cfg, 0, sizeof(cfg)); cfg.device = f.device;
    int rc = mkp_ctx_create(&cfg, &ctx);
    if (rc != MKP_OK) throw Error(rc, "no usable gfx950 device (libmkpileup has no CPU path)");
    mkp_caller kc; memset(&kc, 0, sizeof(kc)); kc.max_depth = a.max_depth;
    const std::vector<mkp_mod_threshold> per_mod = parse_mod_thresholds(a.mod_thresholds);
    pass_thresholds(ctx, a, a.in_bam.c_str(), (int)sav.size(), sav.data(), per_mod, &kc);
    parse_edge_filter(a, &kc);
    if (!a.ignore.empty()) { uint32_t code; if (!parse_code(a.ignore, &code)) throw Error(MKP_E_INVALID, "failed to parse mod code " + a.ignore);
      kc.numeric_mode = 2; kc.collapse_code = code; }
    must(ctx, mkp_set_caller(ctx, &kc));
    must(ctx, mkp_internal_set_extract(ctx, true));
    BedFilter exbed; if (!f.exclude_bed.empty()) exbed = load_bed_for(f.exclude_bed, bd);
    ExtractPlan plan = plan_extract(f, a, bd, have_bed ? &bed : nullptr);
    Admission admission{f, plan};
    TableSink sink(a.out_bed, f.bgzf);
    static const char EXTRACT_HEADER[] = "read_id\tforward_read_position\tref_position\tchrom\tmod_strand\tref_strand\tref_mod_strand\tfw_soft_clipped_start\tfw_soft_clipped_end\tread_length\tcall_prob\tcall_code\t"
                                         "base_qual\tref_kmer\tquery_kmer\tcanonical_base\tmodified_primary_base\tfail\tinferred\twithin_alignment\tflag\n";
    if (!f.no_headers) sink.put(EXTRACT_HEADER, sizeof(EXTRACT_HEADER) - 1);
    // records in file order, a batch per device round
    BamBatch view; view.base = bd.raw.data();
    ExtractCounts c;
    const size_t BATCH = 1 << 15;
    std::vector<mkp_record> recs; std::vector<int64_t> ends;
    std::vector<MkpEvent> ev; std::vector<float> vals; std::vector<uint32_t> n_vals;
    for (size_t r0 = 0; r0 < bd.recs.size() && !admission.done; r0 += BATCH) {
      select_records(f, plan, bd, view, r0, std::min(bd.recs.size(), r0 + BATCH), &recs, &ends, &c);
      if (recs.empty()) continue;
      must(ctx, mkp_internal_sample(ctx, 0, 0, 1, nullptr, recs.data(), (uint32_t)recs.size(), false, &n_vals));
      must(ctx, mkp_internal_extract_fetch(ctx, &ev, &vals));
      const RowSource rows{f, plan, bd, fasta, have_bed ? &bed : nullptr, f.exclude_bed.empty() ? nullptr : &exbed, ctx->tables.st.slots, ev, vals};
      std::string text;
      for (size_t i = 0; i < recs.size() && !admission.done; i++) {
        const MkpReadHdr& h = ctx->sample_shard.hdr[i]; const MkpReadOut& ro = ctx->sample_ro[i];
        const Clips clips = soft_clips(recs[i]);
        switch (admission.judge(recs[i], ends[i], h, ro, clips)) {
          case Admit::Silent: break;
          case Admit::Failed: c.n_failed++; break;
          case Admit::Skipped: c.n_skipped++; break;
          case Admit::Rows: if (record_rows(rows, recs[i], h, ro, clips, &text, &c.n_rows)) c.n_used++; else c.n_skipped++; break;
        }
      }
      sink.put(text.data(), text.size());
    }
    sink.finish();
    if (f.stats) fprintf(stderr, "[mkpileup] extract calls: reads=%llu rows=%llu skipped=%llu failed=%llu\n", (unsigned long long)c.n_used,
        (unsigned long long)c.n_rows, (unsigned long long)c.n_skipped, (unsigned long long)c.n_failed);
    return (int)MKP_OK;
  });
}
