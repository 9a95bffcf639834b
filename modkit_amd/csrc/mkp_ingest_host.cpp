// Device ingest, host side: one shard window of an indexed BAM goes to the GPU COMPRESSED and comes back as a digest.
// Stands in for htslib's IndexedReader::fetch + records() (src/pileup/mod.rs:732-759) and for the tag getters / MmTagInfo::parse
// (src/mod_bam.rs:1388-1470, 900-1000) on the shard path: the BGZF blocks the index lists are uploaded as they sit in the file,
// inflated (mkp_inflate_wave4.hip), CRC-checked, cut into records, filtered and packed into the shard arrays (mkp_ingest.hip) — the
// inflated bytes never exist on the host.  What returns: one MkpReadHdr + tag table + two hashes per kept record (the planner's input),
// the spans of supplementary records (max-depth guard), block status words and error bits.  MM header structures ("layouts") are
// interned on the host from the key hash of each record; the text of a structure seen for the first time is fetched from HBM and
// parsed by the host packer itself.
//
// mkp_internal_ingest_run at the end of the file names the stages in their order; the arithmetic between the launches (upload layout,
// chain table, stage cut, block lists, error mapping, layout interning) is mkp_ingest_stages.hpp, which the CPU tests run as it stands.
#include <atomic>
#include <memory>
#include <thread>

#include "mkp_ingest_dev.hpp"
#include "mkp_ingest_host.hpp"
#include "mkp_ingest_stages.hpp"
#include "mkp_launch.h"
#include <cmath>

using namespace mkp;

#define MKP_INGEST_SPARES 20
namespace {
struct Pinned {
  void* p = nullptr; size_t cap = 0;
  void ensure(size_t n) { if (n <= cap) return; release(); if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { p = nullptr;
      throw Error(MKP_E_NOMEM, "hipHostMalloc failed"); } cap = n; }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
void ok(hipError_t e, const char* what) {
  if (e != hipSuccess) throw Error(MKP_E_DEVICE, std::string("device ingest: ") + what + ": " + hipGetErrorString(e));
}
}  // namespace

struct mkp_dev_ingest {
  int device = 0, prio_mid = 0, prio_lo = 0; hipStream_t stream = nullptr, up_stream = nullptr, crc_stream = nullptr;
    hipEvent_t slot_ev[2] = {nullptr, nullptr}, up_done = nullptr, kev[2] = {nullptr, nullptr}, inf_done = nullptr, crc_done = nullptr;
  std::vector<hipEvent_t> stage_ev;      // upload stages: recorded on up_stream behind a stage's last copy
  std::vector<hipEvent_t> tev;           // timed pairs around the inflate launches of the stages
  // the stages' inflate launches: off the ingest stream, whose chain walks (and the host's one sync per stage) then never wait for an inflate.
  hipStream_t inf_stream[1] = {nullptr};
                                           // (Two such streams, launches alternating, ran two stages side by side at half speed each — the same 76 ms
                                           // for the C3 file — and with the
                                           //  process's seventh stream the chain walks began to queue behind inflate launches: 12 ms syncs.)
  std::vector<hipEvent_t> lay_ev;        // a stage's tables are laid out (ingest stream) -> its inflate may start
  // most rounds a stage may take; 0 = whatever has been issued (tests cap it so that a few-MB BAM goes through several stages)
  static constexpr size_t kStageRounds = 0;
  DevBuf rawcur;
  // the staged path's block table and chain counts: written by the chain kernels straight into page-locked host memory (1.3 MB for a chr20 window) —
  Pinned ztab, chain_cnt;
                            // as copies at the end they waited 8-47 ms on a device busy inflating (round 6 trace); the layout kernel reads the table
                            // back over the link
  // upload staging: two halves of kSlots pieces, 32 MiB page-locked in all (allocating it is part of a fresh context's first ingest: 0.22 ms per MiB)
  static constexpr size_t kPiece = kIngestPiece, kSlots = kIngestSlots;
  Pinned stage, small;                                             // compressed bytes on their way up; tables up / totals + status down
  // the staged path's chain table: the chain kernels read it where it lies (a copy would queue behind the upload's 32 MiB pieces)
  Pinned chain_host;
  DevBuf zin, zblk, zstat, raw, segs, seg_cnt, rec_off, info, sz, extra, tot, dig, parts;
  std::mutex mu;                                                   // one ingest at a time per object
  // buffers the contexts handed back (mkp_internal_ingest_recycle): room for the seven packed arrays and the header buffer of two shards, and four
  std::mutex spare_mu; std::vector<DevBuf> spares;
  DevBuf take(size_t bytes) {
    DevBuf b;
    { std::lock_guard<std::mutex> g(spare_mu); size_t best = SIZE_MAX;
      for (size_t i = 0; i < spares.size(); i++) if (spares[i].cap >= bytes && (best == SIZE_MAX || spares[i].cap < spares[best].cap)) best = i;
      if (best != SIZE_MAX) { b = spares[best]; spares.erase(spares.begin() + (ptrdiff_t)best); return b; } }
    b.ensure(std::max<size_t>(bytes, 256)); return b;
  }
  // everything the object owns, listed once (mkp_internal_ingest_destroy, which is also the failure path of mkp_internal_ingest_create)
  std::vector<DevBuf*> dev_bufs() { return {&zin, &zblk, &zstat, &raw, &segs, &seg_cnt, &rec_off, &info, &sz, &extra, &tot, &dig, &parts, &rawcur}; }
  std::vector<Pinned*> pinned_bufs() { return {&ztab, &chain_cnt, &stage, &small, &chain_host}; }
  std::vector<hipEvent_t> events() const {
    std::vector<hipEvent_t> ev{slot_ev[0], slot_ev[1], up_done, kev[0], kev[1], inf_done, crc_done};
    for (auto* v : {&stage_ev, &tev, &lay_ev}) ev.insert(ev.end(), v->begin(), v->end());
    return ev;
  }
};

// Test hooks (tests/test_gpu_ingest.py; not part of the ABI): smaller upload pieces / stages and a forced capacity of the inflated window, so
// that a few-MB BAM goes through several stages and outgrows its window in the middle of them.  0 = the product's value.
namespace { struct IngestTune { size_t piece = mkp_dev_ingest::kPiece, stage_rounds = mkp_dev_ingest::kStageRounds; uint64_t raw_cap = 0; } g_tune;
            std::atomic<uint64_t> g_reinflated{0}, g_staged_windows{0}; }
extern "C" uint64_t mkp_internal_ingest_reinflated() { return g_reinflated.load(); }   // windows that outgrew their buffer and were inflated again
extern "C" uint64_t mkp_internal_ingest_staged() { return g_staged_windows.load(); }   // windows whose staged inflate stood
extern "C" void mkp_internal_ingest_tune(uint64_t piece_bytes, uint64_t stage_rounds, uint64_t raw_cap_bytes) {
  g_tune.piece = piece_bytes ? std::min<size_t>((size_t)((piece_bytes + 63) & ~63ull), mkp_dev_ingest::kPiece) : mkp_dev_ingest::kPiece;
  g_tune.stage_rounds = stage_rounds ? (size_t)stage_rounds : mkp_dev_ingest::kStageRounds;
  g_tune.raw_cap = raw_cap_bytes;
}

mkp_dev_ingest* mkp_internal_ingest_create(int device) {
  // (a failure half-way hands back the streams and events made so far)
  std::unique_ptr<mkp_dev_ingest, void (*)(mkp_dev_ingest*)> d(new mkp_dev_ingest(), mkp_internal_ingest_destroy); d->device = device;
  // the record kernels' stream goes before the upload and CRC streams: the CRC's thirteen thousand
  // workgroups otherwise hold up the one-workgroup scans that the host waits for (2.6 ms for a 15 us kernel)
  int prio_lo = 0, prio_hi = 0;
  if (hipSetDevice(device) != hipSuccess || hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) return nullptr;
  // (below the contexts' own streams, above the uploads and the CRC)
  const int prio_mid = (prio_lo + prio_hi) / 2 != prio_hi ? (prio_lo + prio_hi) / 2 : prio_hi;
  d->prio_mid = prio_mid; d->prio_lo = prio_lo;   // (streams come from the process-wide pool: 8-10 ms each to create, mkp_ctx.hpp)
  if (pooled_stream_create(&d->stream, device, hipStreamNonBlocking, prio_mid) != hipSuccess
      || pooled_stream_create(&d->up_stream, device, hipStreamNonBlocking, prio_lo) != hipSuccess ||
      pooled_stream_create(&d->crc_stream, device, hipStreamNonBlocking, prio_lo) != hipSuccess) return nullptr;
  for (auto& st : d->inf_stream) if (pooled_stream_create(&st, device, hipStreamNonBlocking, prio_lo) != hipSuccess) return nullptr;
  for (auto& e : d->slot_ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
  if (hipEventCreateWithFlags(&d->up_done, hipEventDisableTiming) != hipSuccess) return nullptr;
  for (auto& e : d->kev) if (hipEventCreate(&e) != hipSuccess) return nullptr;   // (timed: the inflate + chain kernels, for the trace)
  if (hipEventCreateWithFlags(&d->inf_done, hipEventDisableTiming) != hipSuccess
      || hipEventCreateWithFlags(&d->crc_done, hipEventDisableTiming) != hipSuccess) return nullptr;
  return d.release();
}

void mkp_internal_ingest_destroy(mkp_dev_ingest* d) {   // (tolerates an object mkp_internal_ingest_create left half made: null streams and events)
  if (!d) return;
  (void)hipSetDevice(d->device);
  for (DevBuf* b : d->dev_bufs()) b->release();
  for (auto& b : d->spares) b.release();
  for (Pinned* b : d->pinned_bufs()) b->release();
  for (auto& st : d->inf_stream) pooled_stream_release(st, d->device, hipStreamNonBlocking, d->prio_lo);
  pooled_stream_release(d->crc_stream, d->device, hipStreamNonBlocking, d->prio_lo);
  pooled_stream_release(d->stream, d->device, hipStreamNonBlocking, d->prio_mid);
  pooled_stream_release(d->up_stream, d->device, hipStreamNonBlocking, d->prio_lo);
  for (hipEvent_t e : d->events()) if (e) (void)hipEventDestroy(e);
  delete d;
}

DevShard::~DevShard() { for (DevBuf* b : {&d_cigar, &d_cigar16, &d_chunk, &d_seq, &d_tagref, &d_ranks, &d_ml}) b->release(); }

void mkp_internal_ingest_recycle(mkp_dev_ingest* d, DevShard* sh) {
  if (!d || !sh) return;
  std::lock_guard<std::mutex> g(d->spare_mu);
  for (DevBuf* b : {&sh->d_cigar, &sh->d_cigar16, &sh->d_chunk, &sh->d_seq, &sh->d_tagref, &sh->d_ranks, &sh->d_ml}) { if (b->p && d->spares.size() < MKP_INGEST_SPARES) {
      d->spares.push_back(*b); b->p = nullptr; b->cap = 0; } }
}

namespace {

// the A/B knobs of the environment, read once per process
struct IngestKnobs {
  bool trace = false;          // MKP_TRACE_PLAN: the [mkpileup ingest] line with its laps
  bool host_table = false;     // MKP_HOST_BLOCK_TABLE=1: the host walks the BGZF headers (one pread per block), one inflate launch behind the upload
  size_t stage_rounds = 0;     // MKP_STAGE_ROUNDS: most rounds a stage may take (0: the tuned value)
  size_t depth = 1;            // MKP_STAGE_DEPTH: a stage is cut when the one `depth` before it has inflated
  static const IngestKnobs& get() {
    static const IngestKnobs k = [] { IngestKnobs v; v.trace = getenv("MKP_TRACE_PLAN") != nullptr;
      if (const char* e = getenv("MKP_HOST_BLOCK_TABLE")) v.host_table = !strcmp(e, "1");
      if (const char* e = getenv("MKP_STAGE_ROUNDS")) v.stage_rounds = strtoull(e, nullptr, 10);
      if (const char* e = getenv("MKP_STAGE_DEPTH")) v.depth = std::max<size_t>(1, strtoull(e, nullptr, 10));
      return v; }();
    return k;
  }
};

// the laps of the trace line: " <what> <ms since the last lap>", in the order they were taken
struct LapTrace {
  bool on; std::string laps; std::chrono::steady_clock::time_point t_lap;
  LapTrace(bool on_, std::chrono::steady_clock::time_point from) : on(on_), t_lap(from) {}
  void lap(const char* what) { if (on) { auto now = std::chrono::steady_clock::now(); char b[96];
      snprintf(b, sizeof b, " %s %.1f", what, std::chrono::duration<double, std::milli>(now - t_lap).count()); laps += b; t_lap = now; } }
};

void drain_streams(mkp_dev_ingest* d) {   // the ingest, inflate and CRC streams (not the upload's)
  (void)hipStreamSynchronize(d->stream); for (auto& st : d->inf_stream) (void)hipStreamSynchronize(st); (void)hipStreamSynchronize(d->crc_stream);
}

// ---- the four guards of one ingest.  mkp_internal_ingest_run declares them, in this order, behind the ingest object's lock: whichever way
// it is left they run before the lock is released.

// The compressed ranges go up piece by piece — pread into page-locked staging on all cores, async H2D behind them — on a helper thread,
// while the ingest thread walks the block headers (the upload needs the file ranges only).  The upload goes in ROUNDS of kSlots pieces
// (16 MiB), an event behind each (stage_ev; an event that has not been recorded yet does not hold a stream back: the consumer waits for
// the record call itself, wait_past).
// GUARANTEES, whatever way the ingest is left: the uploader has stopped and the copies it queued out of the page-locked staging have
// landed — the next ingest on this object rewrites that staging from its first round on.
class Uploader {
 public:
  Uploader(mkp_dev_ingest* d, const BamSource& bam, const UploadLayout& up) : d_(d), fd_(bam.fd()), path_(bam.path()), up_(up) {
    while (d->stage_ev.size() < up.n_rounds) { hipEvent_t e = nullptr; ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
      d->stage_ev.push_back(e); }
    thread_ = std::thread([this] { run(); });
  }
  ~Uploader() { if (thread_.joinable()) thread_.join(); (void)hipStreamSynchronize(d_->up_stream); }
  Uploader(const Uploader&) = delete; Uploader& operator=(const Uploader&) = delete;
  // blocks until a round behind the first `r_done` has been issued or the uploader has stopped; `stopped_on_error`: it stopped, and early
  struct Progress { size_t rounds_issued; bool stopped_on_error; };
  Progress wait_past(size_t r_done) {
    std::unique_lock<std::mutex> lk(st_mu_); st_cv_.wait(lk, [&] { return rounds_issued_ > r_done || up_finished_; });
    return {rounds_issued_, up_finished_ && up_err_ != nullptr};   // (up_err_ is written before up_finished_ is set under the mutex)
  }
  void join() { thread_.join(); }
  // after join(): what stopped the uploader, if anything did / its wall time
  const Error* error() const { return up_err_.get(); }
  double ms() const { return up_ms_; }

 private:
  void run() {
    auto t_up = std::chrono::steady_clock::now();
    try {
      ok(hipSetDevice(d_->device), "hipSetDevice");
      std::atomic<bool> read_bad{false};
      for (size_t round = 0; round < up_.n_rounds; round++) {
        const size_t half = round & 1, p0 = round * up_.slots, n = up_.round_pieces(round);
        if (round >= 2) ok(hipEventSynchronize(d_->slot_ev[half]), "staging wait");   // the copies that last used this half are done
        uint8_t* base = (uint8_t*)d_->stage.p + half * mkp_dev_ingest::kSlots * mkp_dev_ingest::kPiece;
        HostPool::get().parallel(n, [&](size_t k) {
          const UploadPiece& pc = up_.pieces[p0 + k]; uint8_t* dst = base + k * mkp_dev_ingest::kPiece; size_t got = 0;
          while (got < pc.n) { const ssize_t r = ::pread(fd_, dst + got, pc.n - got, (off_t)(pc.file_off + got)); if (r <= 0) { read_bad = true;
              return; } got += (size_t)r; }
        });
        if (read_bad) throw Error(MKP_E_IO, "read error on " + path_);
        for (const UploadCopy& c : up_.copies(round, mkp_dev_ingest::kPiece))
          ok(hipMemcpyAsync(d_->zin.as<uint8_t>() + c.z_off, base + c.k * mkp_dev_ingest::kPiece, c.bytes, hipMemcpyHostToDevice, d_->up_stream), "H2D");
        ok(hipEventRecord(d_->slot_ev[half], d_->up_stream), "event");
        ok(hipEventRecord(d_->stage_ev[round], d_->up_stream), "event");
        { std::lock_guard<std::mutex> g(st_mu_); rounds_issued_ = round + 1; } st_cv_.notify_all();
      }
      ok(hipEventRecord(d_->up_done, d_->up_stream), "event");
    } catch (const Error& e) { up_err_.reset(new Error(e)); }
    { std::lock_guard<std::mutex> g(st_mu_); up_finished_ = true; } st_cv_.notify_all();
    up_ms_ = ms_since(t_up);
  }
  mkp_dev_ingest* d_; const int fd_; const std::string path_; const UploadLayout& up_;
  std::mutex st_mu_; std::condition_variable st_cv_; size_t rounds_issued_ = 0; bool up_finished_ = false;
  std::unique_ptr<Error> up_err_; double up_ms_ = 0;
  std::thread thread_;
};

// GUARANTEES: an exception that leaves the staged path leaves no kernel of it reading buffers the next ingest rewrites (the ingest, inflate
// and CRC streams are drained)
struct DrainOnThrow { mkp_dev_ingest* d; int n = std::uncaught_exceptions(); ~DrainOnThrow() { if (std::uncaught_exceptions() > n) drain_streams(d); } };

// GUARANTEES: whatever leaves the ingest behind the CRC launch waits for the CRC kernel, which reads buffers the next ingest rewrites
struct CrcJoin { hipEvent_t ev; ~CrcJoin() { (void)hipEventSynchronize(ev); } };

// GUARANTEES: the header buffer, which only this ingest reads, goes back to the spares (or is freed when they are full)
struct SpareBack { mkp_dev_ingest* d; DevBuf b; ~SpareBack() { std::lock_guard<std::mutex> g(d->spare_mu); if (b.p) {
      if (d->spares.size() < MKP_INGEST_SPARES) d->spares.push_back(b);
      else b.release();
    } } };

// what the staged path hands to the rest of the ingest
struct StagedResult {
  bool stood = false;                                  // its inflate launches cover the window: nothing is inflated again
  std::vector<uint32_t> nblk;                          // blocks of each stage (0: a stage that launched nothing)
  hipEvent_t last_inf = nullptr;                       // behind the last stage's inflate
  std::chrono::steady_clock::time_point t_start;       // ms_inflate counts from here when it stood
};

// One ingest of one window: the state the stages share.  mkp_internal_ingest_run (below) calls them in order.
struct IngestRun {
  mkp_dev_ingest* d; const BamSource& bam; const uint32_t tid; const FetchParts& parts; const uint32_t beg, end;
  const std::chrono::steady_clock::time_point t0; const double wait_ms, alloc0;
  std::unique_ptr<DevShard> out{new DevShard()};
  LapTrace trace;
  BamSource::IngestPlan plan; UploadLayout up;
  // from upload_tables on
  size_t nb = 0, ns = 0; uint8_t* sm = nullptr; SmallCarve carve; MkpIngestParams P; std::chrono::steady_clock::time_point t_inf, t_scan;
  uint32_t n_all = 0, n = 0, n_so = 0;
  std::vector<MkpRecDigest> dig; std::vector<int32_t> extra;   // what the pack handed back for the digest stage

  IngestRun(mkp_dev_ingest* d_, const BamSource& bam_, uint32_t tid_, const FetchParts& parts_, std::chrono::steady_clock::time_point t_lock)
      : d(d_), bam(bam_), tid(tid_), parts(parts_), beg((uint32_t)std::max<int64_t>(parts_.front().first, 0)),
        end((uint32_t)std::min<int64_t>(parts_.back().second, 0x7fffffffll)), t0(std::chrono::steady_clock::now()),
        wait_ms(std::chrono::duration<double, std::milli>(t0 - t_lock).count()), alloc0(mkp_tl_alloc_ms()), trace(IngestKnobs::get().trace, t0) {
    out->S.tid = (int32_t)tid; out->S.dev_packed = true;
  }
  void lap(const char* what) { trace.lap(what); }
  MkpIngestTotals* totals() const { return (MkpIngestTotals*)(sm + carve.tot); }

  // ---- 1. the window's file ranges and where they go in the upload buffer; false: nothing under the region (an empty shard)
  bool plan_window() {
    bam.ingest_ranges(tid, parts, &plan);
    if (plan.ranges.empty()) return false;
    lap("ranges");
    ok(hipSetDevice(d->device), "hipSetDevice");
    // (kPiece / kStageRounds unless a test shrank them)
    up = UploadLayout::of(plan.ranges, g_tune.piece, mkp_dev_ingest::kSlots);
    d->zin.ensure(up.zbytes + 64);
    lap("zin");
    d->stage.ensure(2 * mkp_dev_ingest::kSlots * mkp_dev_ingest::kPiece);
    lap("zin+staging");
    return true;
  }

  // ---- 3b. MKP_HOST_BLOCK_TABLE=1: the host walks the block headers beside the upload; the whole window is inflated in one launch behind it
  void host_block_table(Uploader& uploader) {
    bam.ingest_blocks(&plan); out->ms_plan = ms_since(t0); uploader.join(); if (uploader.error()) throw *uploader.error();
    out->ms_upload = uploader.ms();
  }

  // ---- 4. tables: the inflate's block table and the chain segments, through the page-locked small buffer; false: an empty window
  bool upload_tables() {
    bam.bytes_read += plan.comp_total;
    if (plan.raw_total == 0) return false;
    if (plan.blks.size() > 0xfffffff0ull || plan.entries.size() > 0xfffffff0ull) throw Error(MKP_E_UNSUPPORTED,
        "shard window holds too many BGZF blocks; use smaller shards");
    nb = plan.blks.size(); ns = plan.entries.size();
    const std::vector<MkpBgzfBlock> blks = ingest_window_blocks(plan, up.zbase, bam.path());
    const std::vector<MkpSeg> segs = mkp_plan_segments<MkpSeg>(plan);
    lap("segments");
    d->zblk.ensure(nb * sizeof(MkpBgzfBlock)); d->zstat.ensure(nb * 4 + 16); d->raw.ensure(plan.raw_total + 64); d->segs.ensure(ns * sizeof(MkpSeg));
      d->seg_cnt.ensure((ns + 1) * 4); d->tot.ensure(sizeof(MkpIngestTotals));
    carve = SmallCarve::of(nb, ns);
    d->small.ensure(carve.need + carve.need / 4);
    sm = (uint8_t*)d->small.p;
    memcpy(sm + carve.blk, blks.data(), nb * sizeof(MkpBgzfBlock)); memcpy(sm + carve.seg, segs.data(), ns * sizeof(MkpSeg));
    ok(hipMemcpyAsync(d->segs.p, sm + carve.seg, ns * sizeof(MkpSeg), hipMemcpyHostToDevice, d->stream), "H2D");
    ok(hipMemsetAsync(d->tot.p, 0, sizeof(MkpIngestTotals), d->stream), "memset");
    return true;
  }

  // ---- 3c. the whole window in one launch: the host-table path, or a window that outgrew the staged path's estimate
  void inflate_whole_window() {
    t_inf = std::chrono::steady_clock::now();
    ok(hipMemcpyAsync(d->zblk.p, sm + carve.blk, nb * sizeof(MkpBgzfBlock), hipMemcpyHostToDevice, d->stream), "H2D");
    ok(hipMemsetAsync(d->zstat.p, 0xff, nb * 4, d->stream), "memset");
    ok(hipStreamWaitEvent(d->stream, d->up_done, 0), "wait for the upload");
    // ---- inflate + CRC
    ok(hipEventRecord(d->kev[0], d->stream), "event");
    ok(mkp_launch_inflate_auto(d->stream, d->zin.as<uint8_t>(), d->zblk.as<MkpBgzfBlock>(), (uint32_t)nb, d->raw.as<uint8_t>(),
        d->zstat.as<uint32_t>()), "inflate launch");
    // the CRC-32 of every block runs on a stream of its own, beside the record kernels below: its verdict — and the decoders'
    // status words it is OR-ed into — is only read when something has gone wrong, or at the very end (throw_if_corrupt)
    ok(hipEventRecord(d->inf_done, d->stream), "event");
    ok(hipStreamWaitEvent(d->crc_stream, d->inf_done, 0), "wait for the inflate");
    ok(mkp_launch_crc32(d->crc_stream, d->zin.as<uint8_t>(), d->zblk.as<MkpBgzfBlock>(), (uint32_t)nb, d->raw.as<uint8_t>(),
        d->zstat.as<uint32_t>()), "crc launch");
  }
  // ---- the staged inflate stood: the record kernels read what the stages' inflate launches wrote
  void await_staged_inflate(const StagedResult& staged) {
    t_inf = staged.t_start;
    (void)copy_stage();   // (this thread's page-locked copy staging, needed for the digest: allocated while the last stages inflate)
    if (staged.last_inf) ok(hipStreamWaitEvent(d->stream, staged.last_inf, 0), "wait for the inflate");
    ok(hipEventRecord(d->kev[0], d->stream), "event");
  }

  // ---- 5. record chains: count the records of every segment; the block status words and the totals come back behind it (one sync)
  void count_records(const StagedResult& staged) {
    memset(&P, 0, sizeof(P));
    P.raw_len = plan.raw_total; P.tid = (int32_t)tid; P.beg = (int32_t)std::min<uint32_t>(beg, 0x7fffffffu);
      P.end = (int32_t)std::min<uint32_t>(end, 0x7fffffffu); P.n_ref = (int32_t)bam.ref_names.size(); P.n_seg = (uint32_t)ns;
    ok(mkp_launch_ingest_count(d->stream, d->raw.as<uint8_t>(), &P, d->segs.as<MkpSeg>(), d->seg_cnt.as<uint32_t>(), d->tot.as<MkpIngestTotals>()),
        "count launch");
    ok(hipEventRecord(d->kev[1], d->stream), "event");
    ok(hipMemcpyAsync(sm + carve.stat, d->zstat.p, nb * 4, hipMemcpyDeviceToHost, d->crc_stream), "D2H");
    ok(hipEventRecord(d->crc_done, d->crc_stream), "event");
    // the decoders' own status (low byte; the CRC kernel may be OR-ing bit 8 in meanwhile)
    ok(hipMemcpyAsync(sm + carve.stat0, d->zstat.p, nb * 4, hipMemcpyDeviceToHost, d->stream), "D2H");
    ok(hipMemcpyAsync(totals(), d->tot.p, sizeof(MkpIngestTotals), hipMemcpyDeviceToHost, d->stream), "D2H");
    ok(hipStreamSynchronize(d->stream), "inflate sync");
    out->ms_inflate = ms_since(t_inf);
    lap("count+sync");
    // (staged: the stages' inflate launches + the chain kernels)
    const double staged_kernel_ms = staged.stood ? staged_inflate_span(staged) : 0;
    { float kms = 0; if (hipEventElapsedTime(&kms, d->kev[0], d->kev[1]) == hipSuccess) out->ms_kernel = kms + staged_kernel_ms; }
    bam.bytes_inflated += plan.raw_total; bam.bytes_inflated_device += plan.raw_total;
  }
  // the stages' inflate launches may overlap: what is reported is the span from the first launch's start to the last one's end
  double staged_inflate_span(const StagedResult& staged) {
    size_t j0 = SIZE_MAX; float span = 0;
    for (size_t j = 0; j < staged.nblk.size(); j++) if (staged.nblk[j]) { if (j0 == SIZE_MAX) j0 = j; float b = 0;
      if (hipEventElapsedTime(&b, d->tev[2 * j0], d->tev[2 * j + 1]) == hipSuccess) span = std::max(span, b);
      if (trace.on) { float a = 0; (void)hipEventElapsedTime(&a, d->tev[2 * j0], d->tev[2 * j]); char t[64];
        snprintf(t, sizeof t, " {inflate %zu: %.1f-%.1f}", j, a, b); trace.laps += t; } }
    return span;
  }

  // block decoder status / CRC verdict: a corrupt block is what gets reported, whatever the record kernels made of its bytes
  void throw_if_corrupt() {
    ok(hipEventSynchronize(d->crc_done), "crc sync");
    const uint32_t* st = (const uint32_t*)(sm + carve.stat);
    for (size_t i = 0; i < nb; i++) if (st[i] != 0) throw Error(MKP_E_IO, "corrupt BGZF data in " + bam.path() +
        ((st[i] & 0x100u)
            ? " (CRC32 mismatch" : " (decoder status " + std::to_string(st[i] & 0xffu)) + ", block at " + std::to_string(plan.blks[i].coff) + ")");
  }
  void check_error_bits() { const uint32_t err = totals()->err; if (err) throw_if_corrupt(); ingest_throw_error_bits(err, bam.path()); }
  // ---- 5b. a block that did not inflate: nothing behind it is worth parsing
  void check_inflated() {
    const uint32_t* st0 = (const uint32_t*)(sm + carve.stat0); bool bad = false; for (size_t i = 0; i < nb && !bad; i++) bad = (st0[i] & 0xffu) != 0;
    if (bad) throw_if_corrupt();
    check_error_bits();
  }

  // ---- 6. records: offsets, checks + region test + aux walk, sizes -> offsets
  void parse_records() {
    t_scan = std::chrono::steady_clock::now();
    n_all = totals()->n_all;
    P.rec_cap = std::max<uint32_t>(n_all, 1u);
    d->rec_off.ensure((size_t)P.rec_cap * 8); d->info.ensure((size_t)P.rec_cap * sizeof(MkpRecInfo)); d->sz.ensure(7 * (size_t)P.rec_cap * 4);
      d->extra.ensure(2 * (size_t)P.rec_cap * 4);
    const int32_t* d_parts = nullptr;
    if (parts.size() > 1) {   // the windows of a multi-part fetch, next to the params
      std::vector<int32_t> pv; pv.reserve(2 * parts.size()); for (auto& pr : parts) { pv.push_back((int32_t)std::max<int64_t>(pr.first, 0));
        pv.push_back((int32_t)std::min<int64_t>(pr.second, 0x7fffffffll)); }
      d->parts.ensure(pv.size() * 4); ok(hipMemcpyAsync(d->parts.p, pv.data(), pv.size() * 4, hipMemcpyHostToDevice, d->stream), "H2D");
        ok(hipStreamSynchronize(d->stream), "sync");
      P.n_parts = (uint32_t)parts.size(); d_parts = d->parts.as<int32_t>();
    }
    ok(mkp_launch_ingest_parse(d->stream, d->raw.as<uint8_t>(), &P, d_parts, d->segs.as<MkpSeg>(), d->seg_cnt.as<uint32_t>(),
        d->rec_off.as<unsigned long long>(), d->info.as<MkpRecInfo>(), d->sz.as<uint32_t>(),
                               d->extra.as<int32_t>(), d->tot.as<MkpIngestTotals>()), "parse launch");
    ok(hipMemcpyAsync(totals(), d->tot.p, sizeof(MkpIngestTotals), hipMemcpyDeviceToHost, d->stream), "D2H");
    ok(hipStreamSynchronize(d->stream), "parse sync");
    check_error_bits();
    n = totals()->n_kept; n_so = totals()->n_sample_only;
  }

  // ---- 7. pack: the shard's seven arrays (from the spares where one fits), then — into `d_hdr` — the headers, and the digest back
  void take_packed_arrays() {
    const MkpIngestTotals* tot = totals(); const uint32_t n_pk = n + n_so;
    out->d_cigar = d->take((tot->cigar_words + 16) * 4); out->d_cigar16 = d->take((tot->cigar16_entries + 16) * 2); out->d_chunk = d->take((tot->chunk_pairs + 4) * 8); out->d_seq = d->take(tot->seq_bytes + 64);
    out->d_tagref = d->take(((size_t)n_pk * MKP_MAX_TAGS + 1) * sizeof(MkpTagRef)); out->d_ranks = d->take((tot->ml_bytes + 16) * 4);
      out->d_ml = d->take(tot->ml_bytes + 64);
  }
  size_t hdr_bytes() const { return ((size_t)(n + n_so) + 1) * sizeof(MkpReadHdr); }
  void pack_and_fetch_digest(const DevBuf& d_hdr) {
    MkpIngestTotals* tot = totals(); ShardHost& S = out->S; const uint32_t n_pk = n + n_so;
    d->dig.ensure(((size_t)n_pk + 1) * sizeof(MkpRecDigest));
    ok(mkp_launch_ingest_pack(d->stream, d->raw.as<uint8_t>(), P.rec_cap, d->info.as<MkpRecInfo>(), d->sz.as<uint32_t>(), d_hdr.as<MkpReadHdr>(),
        out->d_cigar.as<uint32_t>(), out->d_cigar16.as<uint16_t>(), out->d_chunk.as<uint32_t>(),
                              out->d_seq.as<uint8_t>(), out->d_tagref.as<MkpTagRef>(), out->d_ranks.as<uint32_t>(), out->d_ml.as<uint8_t>(),
                                  d->dig.as<MkpRecDigest>(), d->tot.as<MkpIngestTotals>()), "pack launch");
    S.hdr.resize(n); S.so_hdr.resize(n_so); S.tagref.resize((size_t)n_pk * MKP_MAX_TAGS); S.name_hash.resize(n);
    dig.resize(n_pk); extra.resize(2 * (size_t)tot->n_extra);
    // (into pageable vectors through the library's page-locked staging: handed these directly, the runtime pins them in place, and their
    //  release — with the shard — stalls every queue of the process; mkp_ctx.hpp)
    d2h_copy(S.hdr.data(), d_hdr.p, (size_t)n * sizeof(MkpReadHdr), d->stream);
    d2h_copy(S.so_hdr.data(), d_hdr.as<MkpReadHdr>() + n, (size_t)n_so * sizeof(MkpReadHdr), d->stream);
    if (n_pk) { d2h_copy(S.tagref.data(), out->d_tagref.p, (size_t)n_pk * MKP_MAX_TAGS * sizeof(MkpTagRef), d->stream);
                d2h_copy(dig.data(), d->dig.p, (size_t)n_pk * sizeof(MkpRecDigest), d->stream); }
    d2h_copy(extra.data(), d->extra.p, extra.size() * 4, d->stream);
    ok(hipMemcpyAsync(tot, d->tot.p, sizeof(MkpIngestTotals), hipMemcpyDeviceToHost, d->stream), "D2H");
    ok(hipStreamSynchronize(d->stream), "pack sync");
    check_error_bits();
    throw_if_corrupt();
    out->ms_pack = ms_since(t_scan);
    lap("parse+pack");
  }

  // ---- 8. digest -> what the planner reads: layout ids (this shard's own table; mkp_internal_shard_attach maps them into the context's), flags.
  // A structure not seen in this shard yet: its record comes back from HBM (two copies: the window's record table once, then the record)
  void intern_layouts() {
    auto t_dig = std::chrono::steady_clock::now();
    const MkpIngestTotals* tot = totals(); ShardHost& S = out->S;
    S.n_calls = tot->n_calls; S.dev_n_ranks = tot->n_calls; S.dev_n_ml = tot->n_ml_used;
    for (size_t k = 0; k < extra.size(); k += 2) S.extra_spans.push_back({extra[k], extra[k + 1]});
    ingest_intern_layouts(S, out->layouts, dig, n, n_so, n_all,
        [&](uint64_t wi) { if (out->info_host.empty()) { out->info_host.resize(n_all);
            d2h_copy(out->info_host.data(), d->info.p, (size_t)n_all * sizeof(MkpRecInfo), d->stream); }
          return out->info_host[wi]; },
        [&](const MkpRecInfo& ri, std::vector<uint8_t>* rec) { rec->resize((size_t)ri.bs + 4);
          ok(hipMemcpyAsync(rec->data(), d->raw.as<uint8_t>() + (ri.core - 4), rec->size(), hipMemcpyDeviceToHost, d->stream), "D2H (record)");
          ok(hipStreamSynchronize(d->stream), "sync"); });
    std::vector<MkpRecInfo>().swap(out->info_host);
    out->ms_digest = ms_since(t_dig);
    lap("digest");
  }

  // ---- 9. the shard's counters and times, and the trace line
  void report() {
    out->n_blocks = nb; out->n_segments = ns; out->n_records = n_all; out->raw_bytes = plan.raw_total; out->comp_bytes = plan.comp_total;
    out->ms_total = ms_since(t0); out->ms_alloc = mkp_tl_alloc_ms() - alloc0; out->ms_wait = wait_ms;
    if (trace.on) fprintf(stderr,
        "[mkpileup ingest] tid %u [%u, %u) in %zu window(s): %zu blocks, %zu segments, %u records (%u kept), %.1f MB -> %.1f MB; plan %.1f upload %.1f inflate+chains %.1f (kernels %.1f) parse+pack %.1f digest %.1f total %.1f ms, of which hipMalloc/hipFree %.1f; began at %.1f; laps:%s\n",
        tid, beg, end, parts.size(), nb, ns, n_all, n, plan.comp_total / 1e6, plan.raw_total / 1e6, out->ms_plan, out->ms_upload, out->ms_inflate,
            out->ms_kernel, out->ms_pack, out->ms_digest, out->ms_total, out->ms_alloc,
        std::chrono::duration<double,
            std::milli>(t0.time_since_epoch()).count() - 1000.0 * std::floor(std::chrono::duration<double>(t0.time_since_epoch()).count() / 100.0) * 100.0,
            trace.laps.c_str());
  }
};

// ---- 3a. the STAGED path: the window goes up in rounds of 16 MiB, cut into STAGES as they arrive, and a stage's blocks are found, laid out
// and inflated while the next stage is still on its way (round 4: whole upload, then block table, then one inflate launch — the GPU idle for
// the 40-90 ms of the upload, the host idle for the inflate).  A stage is every round that has been issued when the ingest thread gets to
// it — so the stages grow with what the upload delivered while the stages before were inflating (C3: 16, ~30, ~100, ~120, ~190, ~250 MiB
// ...).  An inflate launch takes whole multiples of one block's latency (4.4 ms with 4 096 one-wave workgroups resident), so few large
// launches beat many equal ones: seven 128 MiB stages took 77 ms of inflate for the C3 file, one launch of everything 58 — but only after
// the whole 30 ms upload.  `stage_rounds` caps a stage (tests).
// The device walks the BGZF headers of the uploaded bytes, one thread per chain between block starts the index knows (round 4 walked them
// on the host with one pread per block: 54 000 preads, 40-90 ms beside an upload that wants the same cores).  Per stage, on the ingest
// stream: wait for the stage's last copy; walk its chains (count -> scan; ONE host sync for the block count, which sizes the launches);
// write its MkpZBlk entries; mkp_bgzf_layout turns them into the inflate's table behind a device-side cursor of the inflated window;
// inflate; CRC on a stream of its own.  The inflated size is not known before the last stage: the window buffer is sized at 6 x the
// compressed bytes and the layout kernel reports an overflow, on which the whole window is inflated again into an exact allocation
// (IngestRun::inflate_whole_window).
struct StagedInflate {
  IngestRun& run; Uploader& uploader; mkp_dev_ingest* d;
  std::vector<BamSource::IngestChain> chains; std::vector<uint64_t> chain_zend; MkpZChain* zc = nullptr;
  IngestStages stages; std::vector<hipEvent_t> inf_end;
  uint64_t raw_cap = 0; size_t blk_cap = 0, blkbase = 0, r_done = 0;
  uint32_t* h_small = nullptr;   // [0] error bits, [1] blocks of the stage; [2..3] the cursor of the inflated window (at the end)
  StagedResult res;
  struct Stage { size_t j, c0, n; uint32_t* cnt; uint32_t nblk; bool outgrown; };   // cnt: the stage's counts -> offsets, its total behind them

  StagedInflate(IngestRun& run_, Uploader& up_) : run(run_), uploader(up_), d(run_.d) {}

  StagedResult go() {
    prepare();
    const size_t stage_rounds = IngestKnobs::get().stage_rounds ? IngestKnobs::get().stage_rounds : g_tune.stage_rounds;
    for (size_t j = 0; r_done < run.up.n_rounds; j++) {
      Stage s;
      if (!cut_stage(j, stage_rounds, &s)) break;   // (the uploader stopped early: its error is reported in finish)
      count_blocks(&s);
      grow_block_tables(s);
      if (s.nblk) launch_stage(s);
    }
    run.lap("stages issued");
    finish();
    return std::move(res);
  }

  // the chain table, the window and the tables the stages append to
  void prepare() {
    run.bam.ingest_chains(run.plan, &chains);
    const size_t nc = chains.size(), n_rounds = run.up.n_rounds;
    run.lap("chains");
    if (nc > 0xfffffff0ull) throw Error(MKP_E_UNSUPPORTED, "shard window holds too many BGZF chains; use smaller shards");
    // the chain table is written into page-locked memory and read from there by the chain kernels (115 KB for a chr20 window): as a copy it
    // waited on the copy engine behind the upload pieces already queued — 44 ms in which no stage could start (round 6 trace)
    d->chain_host.ensure(std::max<size_t>(nc, 1) * sizeof(MkpZChain));
    zc = (MkpZChain*)d->chain_host.p;
    ingest_chain_table(run.plan, chains, run.up.zbase, zc, &chain_zend);
    run.out->ms_plan = ms_since(run.t0);
    run.lap("chain table");
    // the window's capacity as the layout kernel enforces it: a block that would end behind it gets no room at all (out_len 0: the inflate and
    // the CRC of its stage touch nothing), the overflow bit goes up, and the stages after it only build their tables
    raw_cap = g_tune.raw_cap ? g_tune.raw_cap : std::max<uint64_t>(d->raw.cap, run.plan.comp_total * 6 + (64ull << 20));
    d->raw.ensure(raw_cap); run.lap("raw window"); d->chain_cnt.ensure((nc + n_rounds + 2) * 4); d->tot.ensure(sizeof(MkpIngestTotals));
      d->rawcur.ensure(16);
    d->small.ensure(4096);
    h_small = (uint32_t*)d->small.p;
    run.lap("small buffers + events");   // (a temporary: through the library's page-locked staging, mkp_ctx.hpp)
    ok(hipMemsetAsync(d->tot.p, 0, sizeof(MkpIngestTotals), d->stream), "memset");
    ok(hipMemsetAsync(d->rawcur.p, 0, 16, d->stream), "memset");
    blk_cap = std::max<size_t>({d->zblk.cap / sizeof(MkpBgzfBlock), d->ztab.cap / sizeof(MkpZBlk), (size_t)(run.plan.comp_total / 8192 + 4096)});
    d->zblk.ensure(blk_cap * sizeof(MkpBgzfBlock)); d->ztab.ensure(blk_cap * sizeof(MkpZBlk)); d->zstat.ensure(blk_cap * 4 + 16);
    blk_cap = std::min({d->zblk.cap / sizeof(MkpBgzfBlock), d->ztab.cap / sizeof(MkpZBlk), (d->zstat.cap - 16) / 4});
    res.t_start = std::chrono::steady_clock::now();
    run.lap("buffers");
  }

  // step 1: the rounds this stage takes and the chains that end inside them; false: no round is left to take
  bool cut_stage(size_t j, size_t stage_rounds, Stage* s) {
    // pacing: a stage is cut when the one before it has inflated — cut earlier it would be a smaller one (with one stage queued behind the
    // running one, MKP_STAGE_DEPTH=2, the C3 file took 5-6 launches and 73-76 ms of inflate; so: 4 launches, 66-70 ms, ~1 ms idle between them)
    const size_t depth = IngestKnobs::get().depth, n_rounds = run.up.n_rounds;
    if (inf_end.size() >= depth) ok(hipEventSynchronize(inf_end[inf_end.size() - depth]), "stage pacing");
    const Uploader::Progress got = uploader.wait_past(r_done);
    size_t r_now = got.rounds_issued;
    if (run.trace.on) { char b[64]; snprintf(b, sizeof b, " [s%zu: rounds %zu-%zu, issued", j, r_done, r_now); run.lap(b); }
    if (got.stopped_on_error || r_now <= r_done) return false;
    if (stage_rounds && r_now - r_done > stage_rounds) r_now = r_done + stage_rounds;
    ok(hipStreamWaitEvent(d->stream, d->stage_ev[r_now - 1], 0), "wait for the upload rounds");
    // (the stage's events are created as the stages come: their number is not known ahead)
    while (d->tev.size() < 2 * (j + 1)) { hipEvent_t e = nullptr; ok(hipEventCreate(&e), "event"); d->tev.push_back(e); }
    while (d->lay_ev.size() < j + 1) { hipEvent_t e = nullptr; ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
      d->lay_ev.push_back(e); }
    const size_t c0 = stages.c0[j], c1 = ingest_stage_cut(chain_zend, c0, run.up.round_end_z[r_now - 1], r_now == n_rounds);
    stages.c0.push_back(c1); stages.nblk.push_back(0); r_done = r_now;
    *s = {j, c0, c1 - c0, (uint32_t*)d->chain_cnt.p + stages.cnt_at(j), 0, false};
    return true;
  }

  // step 2: count the stage's blocks — the stage's ONE host sync; its answer sizes the launches
  void count_blocks(Stage* s) {
    ok(mkp_launch_bgzf_chain_count(d->stream, d->zin.as<uint8_t>(), zc + s->c0, (uint32_t)s->n, s->cnt, d->tot.as<uint32_t>()), "block table launch");
    ok(hipMemcpyAsync(h_small, d->tot.p, 4, hipMemcpyDeviceToHost, d->stream), "D2H");
      ok(hipMemcpyAsync(h_small + 1, s->cnt + s->n, 4, hipMemcpyDeviceToHost, d->stream), "D2H");
    ok(hipStreamSynchronize(d->stream), "block table sync");
    run.lap("count");
    if (h_small[0] & (MKP_ZE_BAD | MKP_ZE_CHAIN)) throw Error(MKP_E_IO,
        "bad BGZF block in " + run.bam.path() + " (or the index does not match the file)");
    // an earlier stage ran out of window: the rest is inflated in one launch, into an exact allocation
    s->outgrown = (h_small[0] & MKP_ZE_RAWCAP) != 0;
    s->nblk = h_small[1]; stages.nblk[s->j] = s->nblk;
    if (blkbase + s->nblk > 0xfffffff0ull) throw Error(MKP_E_UNSUPPORTED, "shard window holds too many BGZF blocks; use smaller shards");
  }

  // step 3: a window of unusually small blocks: the tables grow, keeping what the stages before wrote
  void grow_dev(DevBuf& b, size_t need, size_t keep) {
    DevBuf nb; nb.ensure(need); ok(hipStreamSynchronize(d->stream), "sync"); for (auto& st : d->inf_stream) ok(hipStreamSynchronize(st), "sync");
      ok(hipStreamSynchronize(d->crc_stream), "sync");
    if (keep) ok(hipMemcpy(nb.p, b.p, keep, hipMemcpyDeviceToDevice), "D2D"); b.release(); b = nb; nb.p = nullptr; nb.cap = 0;
  }
  void grow_block_tables(const Stage& s) {
    if (blkbase + s.nblk <= blk_cap) return;
    const size_t want = std::max<size_t>(2 * blk_cap, blkbase + s.nblk + 4096);
    grow_dev(d->zblk, want * sizeof(MkpBgzfBlock), blkbase * sizeof(MkpBgzfBlock));
    { Pinned nt; nt.ensure(want * sizeof(MkpZBlk));
      ok(hipStreamSynchronize(d->stream), "sync"); if (blkbase) memcpy(nt.p, d->ztab.p, blkbase * sizeof(MkpZBlk)); d->ztab.release();
      d->ztab = nt; }
    grow_dev(d->zstat, want * 4 + 16, blkbase * 4); blk_cap = want;
  }

  // step 4: table write, layout and status reset on the ingest stream; the inflate on a stream of its own; the CRC behind it on a third
  void launch_stage(const Stage& s) {
    const size_t j = s.j; const uint32_t nblk = s.nblk;
    MkpZBlk* ztab = (MkpZBlk*)d->ztab.p + blkbase; MkpBgzfBlock* zblk = d->zblk.as<MkpBgzfBlock>() + blkbase;
      uint32_t* zst = d->zstat.as<uint32_t>() + blkbase;
    ok(mkp_launch_bgzf_chain_write(d->stream, d->zin.as<uint8_t>(), zc + s.c0, (uint32_t)s.n, s.cnt, nblk, ztab, d->tot.as<uint32_t>()),
        "block table launch");
    ok(mkp_launch_bgzf_layout(d->stream, ztab, nblk, d->rawcur.as<unsigned long long>(), raw_cap, zblk, d->tot.as<uint32_t>()), "layout launch");
    ok(hipMemsetAsync(zst, 0xff, (size_t)nblk * 4, d->stream), "memset");
    // the inflate itself goes to a stream of its own: the ingest stream stays free for the next stage's chain walk, the host's one sync per
    // stage no longer waits for an inflate, and the tables come back (and the window is laid out) while the last stages still inflate
    hipStream_t inf = d->inf_stream[0];
    ok(hipEventRecord(d->lay_ev[j], d->stream), "event");
    ok(hipStreamWaitEvent(inf, d->lay_ev[j], 0), "wait for the stage's tables");
    ok(hipEventRecord(d->tev[2 * j], inf), "event");
    if (!s.outgrown) ok(mkp_launch_inflate_auto(inf, d->zin.as<uint8_t>(), zblk, nblk, d->raw.as<uint8_t>(), zst), "inflate launch");
    ok(hipEventRecord(d->tev[2 * j + 1], inf), "event");
    res.last_inf = d->tev[2 * j + 1]; inf_end.push_back(d->tev[2 * j + 1]);
    if (!s.outgrown) {
      ok(hipStreamWaitEvent(d->crc_stream, d->tev[2 * j + 1], 0), "wait for the inflate");
      ok(mkp_launch_crc32(d->crc_stream, d->zin.as<uint8_t>(), zblk, nblk, d->raw.as<uint8_t>(), zst), "crc launch");
    }
    blkbase += nblk;
  }

  // behind the last stage: the uploader's verdict, the whole table back for the window layout the record kernels need (entry points of the
  // chains) and for error reports, and whether the staged inflate stood
  void finish() {
    uploader.join();
    run.lap("uploader joined");
    if (uploader.error()) { drain_streams(d); throw *uploader.error(); }
    run.out->ms_upload = uploader.ms();
    ok(hipMemcpyAsync(h_small, d->tot.p, 4, hipMemcpyDeviceToHost, d->stream), "D2H");
      ok(hipMemcpyAsync(h_small + 2, d->rawcur.p, 8, hipMemcpyDeviceToHost, d->stream), "D2H");
    ok(hipStreamSynchronize(d->stream), "inflate sync");   // (the page-locked table and counts are complete behind it)
    run.lap("tables back + sync");
    res.nblk = stages.nblk;
    const uint32_t zerr = h_small[0]; const std::string& path = run.bam.path();
    if (zerr & (MKP_ZE_BAD | MKP_ZE_CHAIN)) throw Error(MKP_E_IO, "bad BGZF block in " + path + " (or the index does not match the file)");
    if (zerr & MKP_ZE_ISIZE) throw Error(MKP_E_IO, "BGZF block inflates to more than 64 KiB in " + path);
    std::vector<std::vector<BamSource::IngestBlk>> blocks = ingest_chain_blocks(run.plan, chains, run.up.zbase, stages,
        (const uint32_t*)d->chain_cnt.p, (const MkpZBlk*)d->ztab.p);
    run.bam.ingest_layout(&run.plan, chains, blocks);
    run.lap("layout");
    unsigned long long cur; memcpy(&cur, h_small + 2, 8);
    // (a window larger than the estimate: inflated again, into an exact allocation)
    res.stood = !(zerr & MKP_ZE_RAWCAP) && cur == run.plan.raw_total && run.plan.blks.size() == blkbase;
    if (!res.stood) { for (auto& st : d->inf_stream) ok(hipStreamSynchronize(st), "sync"); ok(hipStreamSynchronize(d->crc_stream), "sync");
      if (!(zerr & MKP_ZE_RAWCAP)) throw Error(MKP_E_DEVICE, "internal: the device's window layout differs from the host's");
      g_reinflated++; }
    else g_staged_windows++;
  }
};

}  // namespace

std::unique_ptr<DevShard> mkp_internal_ingest_run(mkp_dev_ingest* d, const BamSource& bam, uint32_t tid, const FetchParts& parts) {
  if (parts.empty()) throw Error(MKP_E_INVALID, "device ingest: no fetch window");
  if (!d) throw Error(MKP_E_DEVICE, "device ingest: no ingest object");
  auto t_lock = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> lock(d->mu);   // (taken first, so released behind every guard below)
  IngestRun run(d, bam, tid, parts, t_lock);
  if (!run.plan_window()) return std::move(run.out);
  Uploader uploader(d, bam, run.up);
  StagedResult staged;
  if (IngestKnobs::get().host_table) run.host_block_table(uploader);
  else { DrainOnThrow drain{d}; staged = StagedInflate(run, uploader).go(); }
  if (!run.upload_tables()) return std::move(run.out);
  if (staged.stood) run.await_staged_inflate(staged); else run.inflate_whole_window();
  run.count_records(staged);
  CrcJoin crc_join{d->crc_done};
  run.check_inflated();
  run.parse_records();
  // (the pack is one stage in three calls only so that the header buffer's guard stands here and not inside a stage: the seven arrays are
  // taken from the spares first, as before, then the header buffer)
  run.take_packed_arrays();
  SpareBack hdr{d, d->take(run.hdr_bytes())};
  run.pack_and_fetch_digest(hdr.b);
  run.intern_layouts();
  run.report();
  return std::move(run.out);
}
