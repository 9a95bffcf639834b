// libmkpileup C ABI (include/mkpileup.h): the context, a shard's plan and residency in HBM (make_resident), the pileup pass over it
// (run_kernels) and its row read-back, BGZF inflate, threshold sampling / summary / extract, region statistics, localize, bedmethyl
// merge and the device bedMethyl reader.  Every kernel is reached through a launcher of mkp_launch.h.  No CPU fallback lives here: rows and counts come from the HIP
// kernels only; without a gfx950 device every compute entry point fails with MKP_E_DEVICE.
#include <atomic>
#include <climits>
#include <memory>
#include <thread>

#include "mkp_bedmethyl_in.hpp"
#include "mkp_ctx.hpp"
#include "mkp_dmr.hpp"
#include "mkp_dmr_reps.hpp"
#include "mkp_dmr_sites.hpp"
#include "mkp_ingest_host.hpp"
#include "mkp_launch.h"
#include "mkp_plan.hpp"

using namespace mkp;

namespace {

// the packed shard's arrays in HBM as the launchers take them: the one place these buffers are cast (built once per pass)
MkpShardArrays shard_arrays(const mkp_ctx* c) {
  MkpShardArrays sh;
  sh.hdr = c->d_hdr.as<MkpReadHdr>(); sh.cigar = c->d_cigar.as<uint32_t>(); sh.cigar16 = c->d_cigar16.as<uint16_t>();
  sh.chunk_pfx = c->d_chunk.as<uint32_t>(); sh.seq = c->d_seq.as<uint8_t>(); sh.tagref = c->d_tagref.as<MkpTagRef>();
  sh.ranks = c->d_ranks.as<uint32_t>(); sh.ml = c->d_ml.as<uint8_t>(); sh.layouts = c->d_layouts.as<MkpLayout>();
  sh.events = c->d_events.as<MkpEvent>(); sh.readout = c->d_readout.as<MkpReadOut>();
  return sh;
}

MkpRowsDev carve_rows(DevBuf& b, uint64_t cap) {
  b.ensure(cap * 44 + 64);
  MkpRowsDev r; uint32_t* p = b.as<uint32_t>();
  r.pos = p; r.info = p + cap; r.code = p + 2 * cap; r.n_valid = p + 3 * cap; r.n_mod = p + 4 * cap; r.n_can = p + 5 * cap; r.n_other = p + 6 * cap;
  r.n_del = p + 7 * cap; r.n_fail = p + 8 * cap; r.n_diff = p + 9 * cap; r.n_nocall = p + 10 * cap;
  return r;
}

template <class V> void upload(DevBuf& b, const V& v) {
  const size_t bytes = v.size() * sizeof(v[0]);
  b.ensure(std::max<size_t>(bytes, 16));
  if (!v.empty()) h2d_copy(b.p, v.data(), bytes);   // (through the library's page-locked staging: mkp_ctx.hpp)
}
}  // namespace

// BGZF inflate on the device: mkp_inflate_wave4, one wave per block — speculative token decode, a scalar walk that only marks the chain,
// all output of a pass placed at once; 4 KiB ring, sixteen waves per CU (round 5; it replaced the five kernels of rounds 2-4 at every
// launch size).  MKP_INFLATE_KERNEL=wave4_8k|wave4_2k picks another ring size (A/B runs; --stats names it).
hipError_t mkp_launch_inflate_auto(hipStream_t st, const uint8_t* in, const MkpBgzfBlock* blks, uint32_t n, uint8_t* out, uint32_t* status) {
  static const char* force = getenv("MKP_INFLATE_KERNEL");
  if (force && !strcmp(force, "wave4_8k")) return mkp_launch_inflate_wave4(st, in, blks, n, out, status, 8);
  if (force && !strcmp(force, "wave4_2k")) return mkp_launch_inflate_wave4(st, in, blks, n, out, status, 2);
  return mkp_launch_inflate_wave4(st, in, blks, n, out, status, 4);
}
namespace {

// d_plane holds the fused reads' call plane, the base plane behind it (as many 8-byte entries each: plane_bytes / 16) and the builder's counter
static MkpCallEnt* call_plane(mkp_ctx* c) { return c->d_plane.as<MkpCallEnt>(); }
static MkpBaseEnt* base_plane(mkp_ctx* c) { return reinterpret_cast<MkpBaseEnt*>(c->d_plane.as<char>() + c->plane_bytes / 2); }

// the plan's arrays into HBM, the buffers the kernels write, the fused reads' call and base planes (built once per resident shard — a re-launch on the
// shard reuses it — and counted in the upload step), the LDS sizes and the key passes
void upload_plan(mkp_ctx* c, const ShardPlan& pl, PlanTrace& trace) {
  const ShardHost& S = c->shard;
  hip_check(hipSetDevice(c->device), "hipSetDevice");
  upload(c->d_hdr, S.hdr);
  if (!S.dev_packed) {
    upload(c->d_cigar, S.cigar); upload(c->d_cigar16, S.cigar16); upload(c->d_chunk, S.chunk_pfx); upload(c->d_seq, S.seq);
    upload(c->d_tagref, S.tagref); upload(c->d_ranks, S.ranks); upload(c->d_ml, S.ml);
  }
  // (device ingest: those arrays were written in HBM by mkp_ingest_pack and handed over by mkp_internal_shard_attach)
  trace.lap("upload: packed reads");
  upload(c->d_layouts, c->tables.dev); upload(c->d_tiles, pl.tiles);
  upload(c->d_read_ids, pl.class_list);
  if (c->has_focus && pl.preplanned) { /* focus bytes, combos, slot bitmap and slot positions went up with the pre-plan */ }
  else if (c->has_focus) { upload(c->d_focus, c->focus); upload(c->d_combos, c->combos); upload(c->d_slotbm, pl.slotbm); }
  else { c->d_focus.ensure(16); c->d_combos.ensure(64); c->d_slotbm.ensure(16); }
  c->d_events.ensure(std::max<uint64_t>(S.n_events_cap, 1) * sizeof(MkpEvent));
  if (c->n_dup_cons) { upload(c->d_dupcons, pl.dup_cons); upload(c->d_dupsegs, pl.dup_segs); }
  c->d_readout.ensure(std::max<size_t>(2 * S.hdr.size(), 1) * sizeof(MkpReadOut));   // second half: second-group summaries of duplex reads
  c->d_misc.ensure(64);
  trace.lap("upload: focus + event buffers");
  if (pl.stream) {
    if (!pl.preplanned) { upload(c->d_slot_pos, pl.slot_pos); upload(c->d_slot_ent, pl.lists.ent); }
    upload(c->d_stiles, pl.stiles);
    const uint32_t nf = c->n_slot_class[0];   // the fused decoder takes work records, the cover kernel keeps a read-id list
    c->d_plane.ensure(c->plane_bytes + 16);   // + the builder's count of the SEQ bytes the decoder reads (MKP_RF_SEQN reads only) behind the entries
    unsigned long long* d_seqn_bytes = reinterpret_cast<unsigned long long*>(c->d_plane.as<char>() + c->plane_bytes);
    hip_check(hipMemsetAsync(d_seqn_bytes, 0, sizeof(unsigned long long), c->stream), "plane counter reset");
    upload(c->d_work, pl.work);
    { std::vector<uint32_t> cover(pl.slot_ids.begin() + nf, pl.slot_ids.end()); upload(c->d_slot_ids, cover); }
    { std::vector<MkpFusedDesc> fd(c->tables.dev.size()); for (size_t i = 0; i < fd.size(); i++) fd[i] = fused_desc(c->tables.dev[i]);
      upload(c->d_fdesc, fd); }
    hip_check(mkp_launch_call_plane(c->stream, c->d_work.as<MkpWork>(), nf, shard_arrays(c), c->d_fdesc.as<MkpFusedDesc>(), call_plane(c),
        base_plane(c), d_seqn_bytes), "call plane launch");
    c->d_cov.ensure(c->cov_bytes + 256); c->d_visits.ensure(std::max<size_t>(S.hdr.size(), 1) * sizeof(MkpVisit));
    // A fused read writes the bytes of the slots it decodes — the same ones on every pass — and the buffer is reused from shard to shard:
    // the whole stream starts as BLANK ("in the column, no feature": the stream kernel skips it and it opens no ref-skip boundary), so that
    // the bytes no read writes tally nothing, on this pass and on every re-launch.
    hip_check(hipMemsetAsync(c->d_cov.p, MKP_FB_BLANK, c->cov_bytes + 256, c->stream), "feature stream prefill");
    hip_check(mkp_stream_set_lds(c->lds_bytes), "hipFuncSetAttribute(max dynamic LDS, stream)");
  }
  if (c->hemi) upload(c->d_hemi_iv, c->hemi_iv);
  // partition keys present in this shard: one accumulate pass each
  c->key_passes.clear();
  if (c->partition_tags.empty()) c->key_passes.push_back(MKP_NO_KEY_FILTER);
  else {
    std::vector<uint8_t> seen(c->key_names.size(), 0);
    for (auto& h : S.hdr) { const uint32_t k = h.flags >> MKP_RF_KEY_SHIFT; if (k < seen.size()) seen[k] = 1; }
    for (uint32_t k = 0; k < seen.size(); k++) if (seen[k]) c->key_passes.push_back(k);
    if (c->key_passes.empty()) c->key_passes.push_back(0);
  }
  hip_check(mkp_pileup_set_lds(c->lds_bytes), "hipFuncSetAttribute(max dynamic LDS)");
  hip_check(hipDeviceSynchronize(), "upload sync");
  trace.lap("upload: slot plan + sync");
}

// algorithmic bytes and the shard's sizes in mkp_stats
void account_bytes(mkp_ctx* c, const ShardPlan& pl) {
  const ShardHost& S = c->shard;
  uint64_t b_reads = 0; for (auto& h : S.hdr) b_reads += 16 + 4ull * h.n_cigar + (h.l_seq + 1) / 2;
  c->stats.n_reads = S.hdr.size(); c->stats.n_tiles = c->n_tiles; c->stats.n_positions = (uint64_t)((int64_t)S.win_end - (int64_t)S.win_start);
  // + 8*events added after the run
  c->stats.alg_bytes_decode = b_reads + (S.dev_packed ? S.dev_n_ranks : S.ranks.size()) * 2ull + (S.dev_packed ? S.dev_n_ml : S.ml.size());
  c->stats.alg_bytes_pileup = b_reads;                                          // + 8*events + 44*rows added after the run
  c->stats.slot_pipeline = pl.stream ? 1u : 0u; c->stats.stream_bytes = 0; c->stats.alg_bytes_agg_survey = 0;
  if (!pl.stream) return;
  // slot pipeline: the decode side also reads the slot positions of every read's span and writes one feature byte per slot and a
  // 32-byte visit record per read; the aggregation kernel reads exactly those (SEQ and CIGAR are read once per pass)
  uint64_t n_rs = 0; for (auto& h : S.hdr) n_rs += h.n_sl;
  c->stats.stream_bytes = n_rs;
  c->stats.alg_bytes_decode += 4ull * n_rs + n_rs + 32ull * S.hdr.size();
  // the fused decoder reads neither a read's whole SEQ nor its rank list, and 2 bytes per CIGAR op (4 of a read with an op longer than
  // 4 095 bases): the 8-byte entry of its plane under each slot (the call plane of a read with calls, the base plane of every other), 4
  // bytes of the base plane per slot without a listed call of a read with calls (a bound: plane_lookup_bytes, mkp_plan.hpp), and the SEQ
  // byte only for a read with a base that is not A/C/G/T (the planes, resolved from SEQ and ranks once per resident shard, are not part of
  // the pass); the plane builder counted those SEQ bytes behind the planes
  unsigned long long seqn_bytes = 0;
  hip_check(hipMemcpyAsync(&seqn_bytes, c->d_plane.as<char>() + c->plane_bytes, sizeof(seqn_bytes), hipMemcpyDeviceToHost, c->stream),
      "plane counter readback");
  hip_check(hipStreamSynchronize(c->stream), "plane counter readback");   // (the shard's own stream: idle here, not the ingest ahead)
  c->stats.alg_bytes_decode = c->stats.alg_bytes_decode - pl.fused_swept + pl.fused_looked_up + seqn_bytes;
  c->stats.alg_bytes_pileup = n_rs + 32ull * S.hdr.size();               // + 44*rows added after the run
  c->stats.alg_bytes_agg_survey = 8ull * n_rs;                            // 8 B per coverage event at a candidate position (+ call events, + 44*rows)
}

// plan the open shard (the stages of mkp_plan.hpp, in their order), keep the plan's scalars for the launches, upload everything
void make_resident(mkp_ctx* c) {
  const auto t0 = std::chrono::steady_clock::now();
  PlanTrace trace(PlanTrace::wanted(), false, t0);   // host planning stages on stderr
  ShardPlan pl;
  const PlanInput in{c->shard, c->tables, c->packer.layouts, c->caller, c->has_focus, c->focus, c->combos, c->iv_starts, c->hemi, c->hemi_off,
      c->hemi_iv, c->cfg.tile_positions, c->partition_tags.size(), c->wplan, PlanKnobs::from_env()};
  find_shared_names(in, pl);
  trace.lap("duplicate-name check");
  build_params(in, pl);
  trace.lap("caller tables + params");
  class_ids(c->shard, c->tables, &pl.class_list, pl.n_class, true);
  trace.lap("decode classes");
  flag_sum_errors(in, pl);
  trace.lap("probability-sum test");
  layout_event_slices(in, pl);
  trace.lap("decode classes + event slices");
  check_sorted_and_depth(in, pl);
  trace.lap(pl.wide ? "sortedness + depth guard (wide tallies)" : "sortedness + depth guard (16-bit tallies)");
  plan_tiles(in, pl);
  trace.lap("slot bitmap + tiles");
  candidate_reads(in, pl);
  plan_name_owners(in, pl, [c](uint32_t r) {   // the one device touch of planning: a member's CIGAR of a device-packed shard
    const MkpReadHdr& h = c->shard.hdr[r]; std::vector<uint32_t> cg(h.n_cigar);
    if (h.n_cigar) { hip_check(hipSetDevice(c->device), "hipSetDevice");
      d2h_copy(cg.data(), shard_arrays(c).cigar + h.cigar_off, (size_t)h.n_cigar * 4, c->stream); }
    return cg; });
  if (!pl.dup_groups.empty()) trace.lap("records sharing a name: owners per interval");
  split_fused_and_cover(in, pl);
  trace.lap("candidate reads per tile");
  memcpy(&c->prm, &pl.prm, sizeof(c->prm));
  if (c->hemi) memcpy(c->hemi_codes, pl.hemi_codes, sizeof(c->hemi_codes));
  memcpy(c->n_class, pl.n_class, sizeof(c->n_class)); memcpy(c->n_slot_class, pl.n_slot_class, sizeof(c->n_slot_class));
  c->read_ids_dec_off = pl.read_ids_dec_off; c->wide = pl.wide; c->slot_mode = pl.stream; c->n_dup_cons = (uint32_t)pl.dup_cons.size();
  c->lds_bytes = pl.lds_bytes; c->n_tiles = pl.n_tiles; c->n_slots_total = pl.n_slots_total; c->cov_bytes = pl.cov_bytes;
  c->stats.pack_ms += ms_since(t0);
  const auto t1 = std::chrono::steady_clock::now();
  build_work_records(in, pl);   // (counted in the upload step, as the plane they address is)
  if (pl.stream) c->plane_bytes = pl.plane_bytes;
  if (trace.on && pl.fused_slots) fprintf(stderr, "[mkpileup plan] fused reads decode %llu of the %llu slots they span (%.3f)\n",
      (unsigned long long)pl.fused_entries, (unsigned long long)pl.fused_slots, (double)pl.fused_entries / (double)pl.fused_slots);
  upload_plan(c, pl, trace);
  c->stats.h2d_ms = ms_since(t1);
  c->resident = true; c->resident_hemi = c->hemi;
  account_bytes(c, pl);
}

// ---- one pileup pass over the resident shard: the stages of run_kernels, in the order they run.  `words` are the pass words in HBM
// (mkp_launch.h) with the runs' look-back words (slot pipeline) or row offsets (tile pipeline) behind them; `sh` the shard's arrays.

// the first guess of the row capacity (a pass that outgrows it is run again with twice as much)
uint64_t first_row_capacity(const mkp_ctx* c) {
  const MkpRunParams& P = c->prm;
  // focus runs: usually one strand rule per focus position and one row per observed code; otherwise two strands per position
  uint64_t guess = c->hemi ? c->n_slots_total * 3 + 4096 : c->has_focus ? c->n_slots_total * std::max<uint32_t>(1u,
      P.numeric_mode == 1 ? P.n_pb : P.n_slots) + 4096 : (uint64_t)c->stats.n_positions * 2 + 1024;
  return std::max<uint64_t>(1u << 16, std::min<uint64_t>(guess * c->key_passes.size(), 1ull << 28));
}

// the buffers with one entry per row run
void size_run_buffers(mkp_ctx* c, uint32_t n_runs) {
  // (slot pipeline: row_off holds the runs' 64-bit look-back words behind a 64-byte header — the pass's cursor / total / error words — so that
  //  ONE memset readies a pass: between two kernels of a 1 ms step every extra fill or copy is a 5-10 us launch of its own)
  c->d_tile_row_off.ensure(MKP_PW_HEADER_BYTES + (size_t)(n_runs + 1) * 8); c->d_tile_row_cnt.ensure((size_t)(n_runs + 1) * 4);
    c->d_tile_dst.ensure((size_t)(n_runs + 1) * 4);
}

// the row buffers at the capacity of this try
void size_row_buffers(mkp_ctx* c) {
  c->prm.row_capacity = (uint32_t)c->row_cap;
  c->rows_src = carve_rows(c->d_rows_src, c->row_cap); c->rows_dst = carve_rows(c->d_rows_dst, c->row_cap);
}

// ready a pass: the one memset, and the parameter block when it changed
void ready_pass(mkp_ctx* c, uint32_t* words, uint32_t n_runs) {
  const MkpRunParams& P = c->prm;
  // rows leave mkp_pileup_stream in genome order (look-back over the runs): the words start at zero, the number of runs is a kernel argument
  hip_check(hipMemsetAsync(words, 0, c->slot_mode ? MKP_PW_HEADER_BYTES + (size_t)(n_runs + 1) * 8 : MKP_PW_HEADER_BYTES, c->stream), "memset");
  c->d_prm.ensure(sizeof(MkpRunParams));
  // (re-launches on a resident shard: unchanged)
  if (c->prm_uploaded.size() != sizeof(MkpRunParams) || c->prm_uploaded_to != c->d_prm.p
      || memcmp(c->prm_uploaded.data(), &P, sizeof(MkpRunParams)) != 0) {
    c->prm_uploaded.assign(reinterpret_cast<const uint8_t*>(&P), reinterpret_cast<const uint8_t*>(&P) + sizeof(MkpRunParams));
      c->prm_uploaded_to = c->d_prm.p;
    hip_check(hipMemcpyAsync(c->d_prm.p, c->prm_uploaded.data(), sizeof(MkpRunParams), hipMemcpyHostToDevice, c->stream), "params H2D");
  }
}

// the decoders: events and read summaries of every read (both pipelines), the feature stream and visits of the slot pipeline
void launch_decoders(mkp_ctx* c, const MkpShardArrays& sh, uint32_t* words) {
  const MkpRunParams& P = c->prm;
  uint32_t* dev_err = words + MKP_PW_ERR;
  if (c->n_dup_cons) hip_check(mkp_launch_dup_restore(c->stream, sh, c->d_dupcons.as<MkpDupCons>(), c->n_dup_cons), "dup restore launch");
  hip_check(mkp_launch_decode(c->stream, sh, c->d_read_ids.as<uint32_t>() + c->read_ids_dec_off, c->n_class, &P, dev_err,
      c->d_focus.as<uint8_t>(), nullptr), "decode launch");
  if (c->hemi) hip_check(mkp_launch_hemi_failed(c->stream, sh, (uint32_t)c->shard.hdr.size(), c->d_slotbm.as<uint32_t>(),
      c->d_hemi_iv.as<uint32_t>(), (uint32_t)c->hemi_iv.size(), P.win_start, P.win_end, dev_err), "hemi failed-reads launch");
  // records answered from another record of their name: their event lists are rebuilt from the owners' (behind every event decoder, in front of
  // whatever consumes events: mkp_cover_reads / mkp_pileup_tiles)
  if (c->n_dup_cons) hip_check(mkp_launch_dup_events(c->stream, sh, c->d_dupcons.as<MkpDupCons>(), c->d_dupsegs.as<MkpDupSeg>(), c->n_dup_cons,
      dev_err), "dup events launch");
  if (c->slot_mode) hip_check(mkp_launch_slots(c->stream, c->d_work.as<MkpWork>(), c->n_slot_class[0], call_plane(c), base_plane(c), sh,
      c->d_slot_ids.as<uint32_t>(), c->n_slot_class[2], c->d_fdesc.as<MkpFusedDesc>(), &P, c->d_slot_pos.as<uint32_t>(),
      c->d_slot_ent.as<MkpSlotEnt>(), c->d_cov.as<uint8_t>(), c->d_visits.as<MkpVisit>()), "slot decode launch");
}

// the accumulate passes: one per partition key present (a single unfiltered pass without --partition-tag)
void launch_accumulate(mkp_ctx* c, const MkpShardArrays& sh, uint32_t* words, uint32_t n_runs) {
  const MkpRunParams& P = c->prm;
  uint32_t* row_off = words + MKP_PW_RUNS;
  for (uint32_t kp = 0; kp < c->key_passes.size(); kp++)
    if (c->slot_mode) hip_check(mkp_launch_stream(c->stream, c->lds_bytes, c->d_visits.as<MkpVisit>(), c->d_cov.as<uint8_t>(), sh.events,
        c->d_stiles.as<MkpSTile>(), c->n_tiles, c->d_prm.as<MkpRunParams>(), c->d_slot_pos.as<uint32_t>(), c->d_focus.as<uint8_t>(),
        c->d_combos.as<MkpCombo>(), &c->rows_src, words + MKP_PW_CURSOR, row_off, words + MKP_PW_ERR, c->key_passes[kp], kp,
        (uint32_t)c->combos.size(), n_runs, P.slot_cap, (P.n_counters + P.n_slots) * (c->wide ? 2u : 1u), c->wide), "stream pileup launch");
    else hip_check(mkp_launch_pileup(c->stream, c->lds_bytes, c->hemi, sh, c->d_tiles.as<MkpTile>(), c->n_tiles, c->d_prm.as<MkpRunParams>(),
        c->d_slotbm.as<uint32_t>(), &c->rows_src, words + MKP_PW_CURSOR, row_off, c->d_tile_row_cnt.as<uint32_t>(), words + MKP_PW_ERR,
        c->key_passes[kp], kp, c->wide), "pileup launch");
}

// the gather: the tiles' row runs into genome order (tile pipeline only)
void launch_gather(mkp_ctx* c, uint32_t* words, uint32_t n_runs) {
  if (c->slot_mode) c->rows_dst = c->rows_src;   // already in genome order
  else hip_check(mkp_launch_gather(c->stream, words + MKP_PW_RUNS, c->d_tile_row_cnt.as<uint32_t>(), c->d_tile_dst.as<uint32_t>(), n_runs,
      words + MKP_PW_ROW_TOTAL, &c->rows_src, &c->rows_dst), "gather launch");
}

// the pass words, back on the host behind everything the pass enqueued
const uint32_t* read_pass_words(mkp_ctx* c, const uint32_t* words) {
  if (!c->h_words && hipHostMalloc(reinterpret_cast<void**>(&c->h_words), 64, hipHostMallocDefault) != hipSuccess) { c->h_words = nullptr;
    throw Error(MKP_E_NOMEM, "hipHostMalloc failed"); }
  hip_check(hipMemcpyAsync(c->h_words, words, 16, hipMemcpyDeviceToHost, c->stream), "D2H");
  hip_check(hipStreamSynchronize(c->stream), "kernel sync");
  return c->h_words;
}

// what the error word says of the pass: true = it stands; false = the rows outgrew their buffers, which are doubled for another try; every
// other error refuses the shard
bool pass_stands(mkp_ctx* c, uint32_t err) {
  if (err & ERR_ROW_CAP) { c->row_cap *= 2; if (c->row_cap > (1ull << 31)) throw Error(MKP_E_NOMEM, "row buffer would exceed 2^31 rows");
    return false; }
  if (err & ERR_EVENT_CAP) throw Error(MKP_E_DEVICE, "internal: event segment overflow");
  if (err & ERR_DUP_MIXED) throw Error(MKP_E_UNSUPPORTED,
      "records sharing a read name inside one interval are answered from the first one's calls (the reference's per-interval cache is keyed by name); here the records one of them is answered from in different intervals disagree in status or observed mod codes, which is not reproduced on the device");
  return true;
}

// the kernel times of a timed pass, from its events
void record_kernel_times(mkp_ctx* c) {
  float a = 0, b = 0, d = 0; hip_check(hipEventElapsedTime(&a, c->ev[0], c->ev[1]), "event");
    hip_check(hipEventElapsedTime(&b, c->ev[1], c->ev[2]), "event");
  if (!c->slot_mode) hip_check(hipEventElapsedTime(&d, c->ev[2], c->ev[3]), "event");   // (the slot pipeline has no gather pass)
  c->stats.decode_kernel_ms = a; c->stats.pileup_kernel_ms = b; c->stats.rows_kernel_ms = 0; c->stats.gather_kernel_ms = d;
    c->stats.kernel_ms = a + b + d;
}

// the pileup pass over the resident shard, tried again with twice the rows while they outgrow their buffers
void run_kernels(mkp_ctx* c, bool time_kernels) {
  // focus runs are the slot pipeline's; the tile kernels of the event pipeline serve runs without focus positions and pileup-hemi only
  if (c->has_focus && !c->hemi && !c->slot_mode) throw Error(MKP_E_INVALID, "internal: a focus run outside the slot pipeline");
  if (c->row_cap == 0) c->row_cap = first_row_capacity(c);
  const bool trace = time_kernels && getenv("MKP_TRACE_PLAN") != nullptr;
  PlanTrace marks(trace, true);
  const uint32_t n_runs = c->n_tiles * (uint32_t)c->key_passes.size();   // row runs: one per (key pass, tile), ordered by key then genome
  size_run_buffers(c, n_runs);
  const MkpShardArrays sh = shard_arrays(c);
  uint32_t* words = c->d_tile_row_off.as<uint32_t>();
  auto mark = [&](int k) { if (time_kernels) hip_check(hipEventRecord(c->ev[k], c->stream), "event"); };
  for (;;) {
    size_row_buffers(c);
    marks.lap("row buffers");
    // (trace runs: what the stream still had queued shows up here, not in the kernels' sync)
    if (trace) { hip_check(hipStreamSynchronize(c->stream), "sync"); marks.lap("stream drained"); }
    ready_pass(c, words, n_runs);
    mark(0);
    launch_decoders(c, sh, words);
    mark(1);
    launch_accumulate(c, sh, words, n_runs);
    mark(2);
    launch_gather(c, words, n_runs);
    if (!c->slot_mode) mark(3);
    marks.lap("launches");
    if (trace && time_kernels) { hip_check(hipEventSynchronize(c->ev[0]), "sync"); marks.lap("first event reached");
      hip_check(hipEventSynchronize(c->ev[2]), "sync"); marks.lap("kernels done (event)"); }
    const uint32_t* h = read_pass_words(c, words);
    marks.lap("sync");
    if (!pass_stands(c, h[MKP_PW_ERR])) continue;
    c->stats.n_rows = h[MKP_PW_ROW_TOTAL];
    if (time_kernels) record_kernel_times(c);
    return;
  }
}

// row columns and per-read outcome counts, device -> host
void fetch_row_columns(mkp_ctx* c) {
  const uint64_t n = c->skip_row_fetch ? 0 : c->stats.n_rows;   // (`--region-stats-only`: the columns stay in HBM, the read summaries still come back)
  const uint32_t* src[11] = {c->rows_dst.pos, c->rows_dst.info, c->rows_dst.code, c->rows_dst.n_valid, c->rows_dst.n_mod, c->rows_dst.n_can,
      c->rows_dst.n_other,
                             c->rows_dst.n_del, c->rows_dst.n_fail, c->rows_dst.n_diff, c->rows_dst.n_nocall};
  c->h_rows.ensure(std::max<uint64_t>(n, 1));
  if (n) { for (int k = 0; k < 11; k++) hip_check(hipMemcpyAsync(c->h_rows.col[k], src[k], n * 4, hipMemcpyDeviceToHost, c->stream), "rows D2H");
    hip_check(hipStreamSynchronize(c->stream), "rows D2H sync"); }
  std::vector<MkpReadOut> ro(c->shard.hdr.size());
  d2h_copy(ro.data(), c->d_readout.p, ro.size() * sizeof(MkpReadOut), c->stream);
  c->n_ok = 0; c->n_bad = 0; uint64_t ev = 0;
  for (auto& r : ro) { if (r.ok) { c->n_ok++; ev += r.n_events; } else c->n_bad++; }
  c->stats.n_events = ev;
}

void fetch_hemi_rows(mkp_ctx* c, mkp_hemi_rows* out) {
  auto t0 = std::chrono::steady_clock::now();
  fetch_row_columns(c);
  const uint64_t n = c->stats.n_rows;
  c->h_hemi_base.resize(n); c->h_hemi_pat[0].resize(n); c->h_hemi_pat[1].resize(n);
  for (uint64_t i = 0; i < n; i++) {   // rows.info = primary base, rows.code = pattern elements a | b << 8
    const uint32_t pb = c->h_rows.col[1][i] & 3u, a = c->h_rows.col[2][i] & 0xffu, b = (c->h_rows.col[2][i] >> 8) & 0xffu;
    c->h_hemi_base[i] = (uint8_t)"ACGT"[pb];
    c->h_hemi_pat[0][i] = a <= MKP_KMAX + 1 ? c->hemi_codes[pb][a] : 0u; c->h_hemi_pat[1][i] = b <= MKP_KMAX + 1 ? c->hemi_codes[pb][b] : 0u;
  }
  c->stats.d2h_ms = ms_since(t0);
  if (out) {
    out->n_rows = n; out->pos = c->h_rows.col[0]; out->primary_base = c->h_hemi_base.data(); out->pattern_pos = c->h_hemi_pat[0].data();
        out->pattern_neg = c->h_hemi_pat[1].data();
    out->n_valid = c->h_rows.col[3]; out->count = c->h_rows.col[4]; out->n_canonical = c->h_rows.col[5]; out->n_other_pattern = c->h_rows.col[6];
    out->n_delete = c->h_rows.col[7]; out->n_fail = c->h_rows.col[8]; out->n_diff = c->h_rows.col[9]; out->n_nocall = c->h_rows.col[10];
    out->processed_records = c->n_ok; out->skipped_records = c->n_bad;
  }
}

void fetch_rows(mkp_ctx* c, mkp_rows* out) {
  auto t0 = std::chrono::steady_clock::now();
  fetch_row_columns(c);
  const uint64_t n = c->skip_row_fetch ? 0 : c->stats.n_rows;
  c->h_strand.resize(n); c->h_motif.resize(n); c->h_key.resize(n);
  host_parallel(n, (size_t)1 << 17, [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) { const uint32_t inf = c->h_rows.col[1][i];
      c->h_strand[i] = "+-."[inf & 3u]; c->h_motif[i] = (int32_t)((inf >> 8) & 0xffu) - 1;
      c->h_key[i] = inf >> 16; } });
  c->key_name_ptrs.clear(); for (auto& k : c->key_names) c->key_name_ptrs.push_back(k.c_str());
  c->stats.d2h_ms = ms_since(t0);
  if (out) {
    out->n_rows = n; out->pos = c->h_rows.col[0]; out->strand = c->h_strand.data(); out->code_repr = c->h_rows.col[2];
      out->motif_idx = c->h_motif.data();
    out->n_valid = c->h_rows.col[3]; out->n_mod = c->h_rows.col[4]; out->n_canonical = c->h_rows.col[5]; out->n_other = c->h_rows.col[6];
    out->n_delete = c->h_rows.col[7]; out->n_fail = c->h_rows.col[8]; out->n_diff = c->h_rows.col[9]; out->n_nocall = c->h_rows.col[10];
    out->processed_records = c->n_ok; out->skipped_records = c->n_bad;
    out->partition_key = c->h_key.data(); out->n_partition_keys = (uint32_t)c->key_name_ptrs.size();
      out->partition_key_names = c->key_name_ptrs.data();
  }
}

// get_stringable_aux (util.rs:670-688): the value of an aux field as the text the reference partitions by
bool aux_stringable(const mkp_record& r, const char* tag, std::string* out) {
  if (!r.data || r.l_data <= 0) return false;
  const size_t fixed = (size_t)r.l_qname + 4 * (size_t)r.n_cigar + ((size_t)std::max(r.l_qseq, 0) + 1) / 2 + (size_t)std::max(r.l_qseq, 0);
  if (fixed > (size_t)r.l_data) return false;
  const uint8_t* a = r.data + fixed; const uint8_t* e = r.data + r.l_data;
  auto width = [](uint8_t ty) -> int { switch (ty) { case 'A': case 'c': case 'C': return 1; case 's': case 'S': return 2;
      case 'i': case 'I': case 'f': return 4;
      case 'd': return 8; default: return -1; } };
  while (a + 3 <= e) {
    const uint8_t ty = a[2]; const uint8_t* v = a + 3; const uint8_t* nx;
    if (ty == 'Z' || ty == 'H') { const uint8_t* z = v; while (z < e && *z) z++; if (z >= e) return false; nx = z + 1; }
    else if (ty == 'B') { if (v + 5 > e) return false; const int w = width(v[0]); uint32_t cnt; memcpy(&cnt, v + 1, 4);
        if (w < 0 || (uint64_t)cnt * (uint64_t)w > (uint64_t)(e - v - 5)) return false; nx = v + 5 + (size_t)cnt * (size_t)w; }
    else { const int w = width(ty); if (w < 0 || v + w > e) return false; nx = v + w; }
    if (a[0] == (uint8_t)tag[0] && a[1] == (uint8_t)tag[1]) {   // first occurrence (bam_aux_get)
      char buf[64];
      switch (ty) {
        case 'Z': case 'H': out->assign((const char*)v, (size_t)(nx - 1 - v)); return true;
        case 'A': out->assign(1, (char)v[0]); return true;
        case 'c': snprintf(buf, sizeof(buf), "%d", (int)(int8_t)v[0]); break;
        case 'C': snprintf(buf, sizeof(buf), "%u", (unsigned)v[0]); break;
        case 's': { int16_t x; memcpy(&x, v, 2); snprintf(buf, sizeof(buf), "%d", (int)x); break; }
        case 'S': { uint16_t x; memcpy(&x, v, 2); snprintf(buf, sizeof(buf), "%u", (unsigned)x); break; }
        case 'i': { int32_t x; memcpy(&x, v, 4); snprintf(buf, sizeof(buf), "%d", x); break; }
        case 'I': { uint32_t x; memcpy(&x, v, 4); snprintf(buf, sizeof(buf), "%u", x); break; }
        default: return false;   // floats print through Rust's Display (shortest round-trip form): not restated; arrays are not stringable
      }
      *out = buf; return true;
    }
    a = nx;
  }
  return false;
}

template <class F> int guarded(mkp_ctx* c, F f) {
  try { f(); return MKP_OK; }
  catch (const Error& e) { if (c) c->err = e.what(); return e.status; }
  catch (const std::bad_alloc&) { if (c) c->err = "out of host memory"; return MKP_E_NOMEM; }
  catch (const std::exception& e) { if (c) c->err = e.what(); return MKP_E_INVALID; }
}

}  // namespace

extern "C" {

const char* mkp_version(void) { return "libmkpileup 0.1 (gfx950)"; }
unsigned mkp_host_threads(void) { return HostPool::get().size(); }
// test hook (tests/test_host_deflate.py; not part of include/mkpileup.h): the host DEFLATE decoder alone, 1 = decoded, 0 = declined
int mkp_internal_host_inflate(const uint8_t* src, size_t clen, uint8_t* dst, size_t dlen) {
  std::vector<uint8_t> padded(clen + 8, 0); if (clen) memcpy(padded.data(), src, clen);
  return hostinf::inflate(padded.data(), clen, dst, dlen) ? 1 : 0;
}

// test hook (tests/test_host_deflate.py): the CRC-32 every inflate path checks a block's bytes with (mkp_crc32.hpp)
uint32_t mkp_internal_crc32(const uint8_t* p, size_t n) { return crc32_of(p, n); }

int mkp_ctx_create(const mkp_config* cfg, mkp_ctx** out) {
  if (!out) return MKP_E_INVALID;
  *out = nullptr;
  mkp_ctx* c = new (std::nothrow) mkp_ctx();
  if (!c) return MKP_E_NOMEM;
  memset(&c->cfg, 0, sizeof(c->cfg)); if (cfg) c->cfg = *cfg;
  memset(&c->stats, 0, sizeof(c->stats));
  c->device = c->cfg.device;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { delete c; return MKP_E_DEVICE; }
  if (c->device < 0 || c->device >= n) { delete c; return MKP_E_DEVICE; }
  // the context's stream runs the short kernels a caller waits for — sampling rounds, the pileup pass — often beside an ingest that fills the
  // chip for tens of milliseconds: it goes first when workgroup slots free up
  { int plo = 0, phi = 0;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceGetStreamPriorityRange(&plo, &phi) != hipSuccess
        || pooled_stream_create(&c->stream, c->device, hipStreamDefault, phi) != hipSuccess) {
      delete c; return MKP_E_DEVICE; } c->stream_prio = phi; }
  // timing events between the kernels of a pass: no system-scope fence when they are recorded (its cache write-back and invalidation sat
  // between the decoder and the kernel that reads what it just wrote; nothing on the host looks at device memory through these events)
  for (auto& e : c->ev) if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) { delete c; return MKP_E_DEVICE; }
  c->caller = CallerCfg();
  *out = c;
  return MKP_OK;
}

void mkp_ctx_destroy(mkp_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (DevBuf* b : {&c->d_vals, &c->d_hdr, &c->d_cigar, &c->d_cigar16, &c->d_seq, &c->d_tagref, &c->d_ranks, &c->d_ml, &c->d_layouts, &c->d_events, &c->d_readout,
      &c->d_focus, &c->d_combos, &c->d_tiles,
                    &c->d_slotbm, &c->d_prm, &c->d_read_ids, &c->d_chunk, &c->d_store, &c->d_hist0, &c->d_hist1, &c->d_sample_cursor, &c->d_take,
                        &c->d_tile_row_off, &c->d_tile_row_cnt, &c->d_tile_dst, &c->d_misc, &c->d_rows_src, &c->d_rows_dst, &c->d_hemi_iv,
                        &c->d_slot_pos, &c->d_slot_ent, &c->d_cov, &c->d_visits, &c->d_stiles, &c->d_slot_ids, &c->d_fdesc, &c->d_work, &c->d_plane,
                        &c->d_zin, &c->d_zout,
                        &c->d_zblk, &c->d_zstat, &c->d_summary, &c->d_bedmask, &c->d_hist64, &c->rstats.d_out, &c->rstats.d_seen,
                        &c->rstats.d_cnt, &c->rstats.d_off, &c->loc.d_tab}) b->release();
  for (auto& kv : c->merge.contigs) for (DevBuf& b : kv.second.buf) b.release();
  for (DevBuf* b : {&c->merge.d_stage, &c->merge.d_cuts, &c->merge.d_counts, &c->merge.d_offsets}) b->release();
  for (auto& kv : c->dmr.ref) kv.second.buf.release();
  for (DevBuf* b : {&c->dmr.d_out, &c->dmr.d_seen, &c->dmr.d_cnt, &c->dmr.d_off, &c->dmr.carry[0].buf, &c->dmr.carry[1].buf}) b->release();
  for (auto& kv : c->dsites.contigs) { kv.second.ref.release(); for (auto& r : kv.second.rows) r.buf.release(); }
  for (auto& kv : c->dreps.contigs) { kv.second.ref.release(); for (auto& r : kv.second.rows) r.buf.release(); }
  { mkp_ctx::BedIn& B = c->bedin;
    for (DevBuf* b : {&B.d_zin, &B.d_text[0], &B.d_text[1], &B.d_blk, &B.d_stat, &B.d_cnt, &B.d_words, &B.d_lines, &B.d_rows, &B.d_runs, &B.d_names})
      b->release();
    for (auto& e : B.ev) if (e) (void)hipEventDestroy(e); }
  for (mkp_ctx::RowTable* t : {static_cast<mkp_ctx::RowTable*>(&c->rstats), static_cast<mkp_ctx::RowTable*>(&c->loc),
      static_cast<mkp_ctx::RowTable*>(&c->merge), static_cast<mkp_ctx::RowTable*>(&c->dmr), static_cast<mkp_ctx::RowTable*>(&c->dsites),
      static_cast<mkp_ctx::RowTable*>(&c->dreps)}) {
    for (DevBuf* b : {&t->d_regions, &t->d_misc, &t->d_lo, &t->d_hi, &t->d_rows}) b->release();
    for (auto& e : t->ev) if (e) (void)hipEventDestroy(e);
  }
  mkp_internal_ingest_destroy(c->ingest); c->ingest = nullptr;
  c->h_rows.release();
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  if (c->h_words) (void)hipHostFree(c->h_words);
  pooled_stream_release(c->stream, c->device, hipStreamDefault, c->stream_prio);   // (drained, then parked for the next context: mkp_ctx.hpp)
  delete c;
}

const char* mkp_last_error(const mkp_ctx* c) { return c ? c->err.c_str() : "no context (is a gfx950 device visible?)"; }

int mkp_set_caller(mkp_ctx* c, const mkp_caller* k) {
  if (!c || !k) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (k->numeric_mode > 2) throw Error(MKP_E_INVALID, "numeric_mode must be 0, 1 or 2");
    CallerCfg cc; cc.default_threshold = k->default_threshold;
    for (int b = 0; b < 4; b++) { cc.per_base[b] = k->per_base_threshold[b]; cc.has_per_base[b] = k->has_per_base[b] != 0; }
    for (uint32_t i = 0; i < k->n_per_mod; i++) cc.per_mod[k->per_mod[i].code_repr] = k->per_mod[i].threshold;
    cc.numeric_mode = k->numeric_mode; cc.collapse_code = k->collapse_code; cc.edge = k->edge_filter != 0; cc.edge_start = k->edge_start;
      cc.edge_end = k->edge_end;
    cc.edge_inverted = k->edge_inverted != 0; cc.force_allow = k->force_allow_implicit != 0; cc.combine_strands = k->combine_strands != 0;
    cc.max_depth = k->max_depth ? k->max_depth : 8000;
    c->caller = cc; c->caller_set = true; c->resident = false;
  });
}

int mkp_set_partition_tags(mkp_ctx* c, const char* const* tags, uint32_t n) {
  if (!c || (!tags && n)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    std::vector<std::string> v;
    for (uint32_t i = 0; i < n; i++) { if (!tags[i] || strlen(tags[i]) != 2) throw Error(MKP_E_INVALID, "SAM tags are two characters");
        if (std::find(v.begin(), v.end(), tags[i]) != v.end()) throw Error(MKP_E_INVALID, "partition tag given twice"); v.push_back(tags[i]); }
    c->partition_tags = v; c->resident = false;
  });
}

int mkp_shard_begin(mkp_ctx* c, const mkp_shard* s) {
  if (!c || !s) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (s->end <= s->start) throw Error(MKP_E_INVALID, "empty shard window");
    if ((uint64_t)s->end > 0x7fffffffull) throw Error(MKP_E_UNSUPPORTED, "reference coordinates beyond 2^31");
    c->shard.clear(); c->shard.tid = s->tid; c->shard.win_start = (int32_t)s->start; c->shard.win_end = (int32_t)s->end;
    c->has_focus = s->focus != nullptr;
    if (c->has_focus) {
      { const size_t nf = (size_t)(s->end - s->start); c->focus.resize(nf); const uint8_t* src = s->focus; uint8_t* dst = c->focus.data();
        host_parallel(nf, (size_t)4 << 20, [&](size_t lo, size_t hi) { memcpy(dst + lo, src + lo, hi - lo); }); }
      if (s->n_combos > 64) throw Error(MKP_E_UNSUPPORTED, "more than 64 motif combos");
      c->combos.assign(s->combos, s->combos + s->n_combos);
      if (c->combos.empty()) { mkp_motif_combo z; memset(&z, 0, sizeof(z)); c->combos.push_back(z); }
    } else { c->focus.clear(); c->combos.clear(); }
    c->shard_open = true; c->resident = false; c->row_cap = 0; c->iv_starts.clear(); c->wplan.valid = false;
    c->key_names.assign(1, "ungrouped");
    memset(&c->stats, 0, sizeof(c->stats));
  });
}

// Ahead of the reads (the device ingest of this shard is still running): everything of the plan that depends on the window alone.
}   // extern "C"
int mkp_internal_shard_preplan(mkp_ctx* c) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->shard_open) throw Error(MKP_E_INVALID, "mkp_shard_begin first");
    c->wplan.valid = false;
    if (!stream_pipeline(c->has_focus, false)) return;
    window_slots(c->shard, c->focus.data(), c->combos, false, true, c->wplan.slotbm, c->wplan.wpfx, c->wplan.slot_pos, c->wplan.lists);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    upload(c->d_focus, c->focus); upload(c->d_combos, c->combos); upload(c->d_slotbm, c->wplan.slotbm); upload(c->d_slot_pos, c->wplan.slot_pos);
    upload(c->d_slot_ent, c->wplan.lists.ent);
    c->wplan.valid = true;
    // a fresh context's first shard: page-locking the row arena costs ~25 ms per 100 MB — here it hides behind the ingest (the caller is
    // about to wait for it); two rows per focus position is what a two-code run can produce at most per strand rule
    if (c->h_rows.cap == 0 && !c->wplan.slot_pos.empty()) c->h_rows.ensure(std::min<size_t>(c->wplan.slot_pos.size() * 2, (size_t)1 << 26));
  });
}
extern "C" {

// The reference's interval grid inside the open shard (ascending interval starts; the last interval ends with the window): only read by the
// duplicate-name rule of the planner — records with one name matter only when they overlap a common interval.  Without it the shard counts
// as one interval.
int mkp_shard_set_intervals(mkp_ctx* c, const uint32_t* starts, uint32_t n) {
  if (!c || (!starts && n)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->shard_open) throw Error(MKP_E_INVALID, "mkp_shard_begin first");
    c->iv_starts.assign(starts, starts + n);
    if (!std::is_sorted(c->iv_starts.begin(), c->iv_starts.end())) throw Error(MKP_E_INVALID, "interval starts must ascend");
  });
}

int mkp_shard_add_records(mkp_ctx* c, const mkp_record* recs, uint32_t n) {
  if (!c || (!recs && n)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->shard_open) throw Error(MKP_E_INVALID, "mkp_shard_begin first");
    auto t0 = std::chrono::steady_clock::now();
    const int32_t tid = c->shard.tid;
    const size_t hdr_before = c->shard.hdr.size();
    pack_records(c->packer, c->shard, recs, n, [tid](const mkp_record& r) { return r.tid == tid && Packer::keep(r); });
    // supplementary records are not tallied but htslib buffers them (BAM_DEF_MASK lets 0x800 through): their spans count for the max-depth guard
    for (uint32_t i = 0; i < n; i++) {
      const mkp_record& r = recs[i];
      if (r.tid != tid || !(r.flag & 2048) || (r.flag & (4 | 256 | 512 | 1024)) || !r.n_cigar || !r.data
          || (uint64_t)r.l_qname + 4ull * r.n_cigar > (uint64_t)std::max(r.l_data,
          0)) continue;
      int64_t len = 0; for (uint32_t k = 0; k < r.n_cigar; k++) { uint32_t w; memcpy(&w, r.data + r.l_qname + 4 * (size_t)k, 4);
          if ((0x18du >> (w & 15u)) & 1u) len += w >> 4; }
      c->shard.extra_spans.push_back({r.pos, (int32_t)std::min<int64_t>((int64_t)r.pos + std::max<int64_t>(len, 1), INT32_MAX)});
    }
    // PartitionKey per kept record (parse_tags_from_record, pileup/mod.rs:626-643): values joined by '_', "missing" for an absent tag
    if (!c->partition_tags.empty()) {
      size_t at = hdr_before;
      for (uint32_t i = 0; i < n; i++) {
        const mkp_record& r = recs[i];
        if (!(r.tid == tid && Packer::keep(r))) continue;
        if (at >= c->shard.hdr.size()) throw Error(MKP_E_INVALID, "internal: packer dropped a kept record");
        std::string key; bool any = false;
        for (size_t t = 0; t < c->partition_tags.size(); t++) { std::string v; const bool got = aux_stringable(r, c->partition_tags[t].c_str(), &v);
          any |= got;
            if (t) key += '_'; key += got ? v : std::string("missing"); }
        uint32_t id = 0;
        if (any) { auto it = std::find(c->key_names.begin() + 1, c->key_names.end(), key); id = (uint32_t)(it - c->key_names.begin());
            if (it == c->key_names.end()) {
              if (c->key_names.size() >= 65535) throw Error(MKP_E_UNSUPPORTED, "more than 65534 partition keys in one shard");
            c->key_names.push_back(key); } }
        c->shard.hdr[at].flags |= id << MKP_RF_KEY_SHIFT;
        at++;
      }
      if (at != c->shard.hdr.size()) throw Error(MKP_E_INVALID, "internal: packer added records that were not kept");
    }
    c->resident = false; c->row_cap = 0;   // the HBM copy and the tile plan belong to the previous record set
    c->stats.pack_ms += ms_since(t0);
  });
}

}   // extern "C"
namespace {
// the shard's own layout ids -> the context's table (shared with the threshold sampler); once per shard
void adopt_layouts(mkp_ctx* c, DevShard* sh) {
  if (sh->layouts_adopted) return;
  const std::vector<uint16_t> map = c->packer.adopt(sh->layouts);
  for (auto* hv : {&sh->S.hdr, &sh->S.so_hdr}) for (auto& h : *hv) if (h.n_tags && !(h.flags & MKP_RF_BAD)) {
    if (h.layout >= map.size()) throw Error(MKP_E_DEVICE, "internal: device ingest layout id out of range");
    h.layout = map[h.layout]; }
  sh->layouts_adopted = true;
}
// the seven arrays the device ingest packs in HBM change hands between the context and a DevShard
void swap_packed_arrays(mkp_ctx* c, DevShard* sh) {
  std::swap(c->d_cigar, sh->d_cigar); std::swap(c->d_cigar16, sh->d_cigar16); std::swap(c->d_chunk, sh->d_chunk); std::swap(c->d_seq, sh->d_seq);
  std::swap(c->d_tagref, sh->d_tagref); std::swap(c->d_ranks, sh->d_ranks); std::swap(c->d_ml, sh->d_ml);
}
void ensure_packed_arrays(mkp_ctx* c) {   // (an empty shard: the kernels still take valid pointers)
  for (DevBuf* b : {&c->d_cigar, &c->d_cigar16, &c->d_chunk, &c->d_seq, &c->d_tagref, &c->d_ranks, &c->d_ml}) b->ensure(16);
}
}  // namespace
int mkp_internal_sample_bind(mkp_ctx* c, DevShard* sh) {
  if (!c || !sh) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!sh->bound) adopt_layouts(c, sh);
    std::swap(c->shard, sh->S);
    swap_packed_arrays(c, sh);
    sh->bound = !sh->bound;
    c->shard_open = sh->bound; c->resident = false; c->wplan.valid = false;
    if (sh->bound) ensure_packed_arrays(c);
  });
}
// Device ingest hand-over (mkp_ingest_host.cpp): the open shard takes the records the device packed.  Their big arrays are swapped into
// the context's device buffers (what those held goes back with `sh`), the digest becomes the host shard, layout ids are mapped into the
// context's table (shared with the threshold sampler).
int mkp_internal_shard_attach(mkp_ctx* c, DevShard* sh) {
  if (!c || !sh) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->shard_open) throw Error(MKP_E_INVALID, "mkp_shard_begin first");
    if (!c->partition_tags.empty()) throw Error(MKP_E_INVALID, "internal: device ingest does not read partition tags");
    if (!c->shard.hdr.empty()) throw Error(MKP_E_INVALID, "internal: the shard already holds host-packed records");
    auto t0 = std::chrono::steady_clock::now();
    if (sh->bound) throw Error(MKP_E_INVALID, "internal: the shard is still bound for sampling");
    adopt_layouts(c, sh);
    const int32_t tid = c->shard.tid, ws = c->shard.win_start, we = c->shard.win_end;
    c->shard = std::move(sh->S); c->shard.tid = tid; c->shard.win_start = ws; c->shard.win_end = we; c->shard.dev_packed = true;
    swap_packed_arrays(c, sh);
    ensure_packed_arrays(c);
    c->resident = false; c->row_cap = 0;
    c->stats.pack_ms += ms_since(t0);
  });
}
extern "C" {

int mkp_shard_run(mkp_ctx* c, mkp_rows* out) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->shard_open) throw Error(MKP_E_INVALID, "mkp_shard_begin first");
    if (!c->caller_set) throw Error(MKP_E_INVALID, "mkp_set_caller first");
    c->hemi = false;
    PlanTrace trace(PlanTrace::wanted());
    if (!c->resident || c->resident_hemi) { c->row_cap = 0; make_resident(c); }
    trace.lap("run: make_resident");
    run_kernels(c, true);
    trace.lap("run: kernels");
    fetch_rows(c, out);
    trace.lap("run: fetch rows");
    if (c->slot_mode) {   // n_events = call features + events of the reads the event decoders took
      c->stats.alg_bytes_pileup += 44ull * c->stats.n_rows;
      c->stats.alg_bytes_agg_survey += 44ull * c->stats.n_rows;
    } else {
      c->stats.alg_bytes_decode += 8ull * c->stats.n_events;
      c->stats.alg_bytes_pileup += 8ull * c->stats.n_events + 44ull * c->stats.n_rows;   // rows leave the accumulate kernel directly
    }
    c->stats.alg_bytes_rows = 0;
  });
}

// process_region_batch (src/pileup/mod.rs:684-716) as ONE call: the intervals of a MultiChromCoordinates with the records the caller's
// reader fetched for them.  Runs of intervals that follow each other on one contig become one resident shard (one pack, one plan, one
// launch sequence, one read-back); the rows come back per interval.
int mkp_batch_run(mkp_ctx* c, const mkp_shard* ivs, uint32_t n_ivs, const mkp_record* recs, uint32_t n_recs, mkp_rows* out) {
  if (!c || (!ivs && n_ivs) || (!recs && n_recs) || (!out && n_ivs)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->caller_set) throw Error(MKP_E_INVALID, "mkp_set_caller first");
    for (auto& v : c->batch_cols) v.clear();
    c->batch_strand.clear(); c->batch_motif.clear(); c->batch_key.clear();
    struct Slice { uint64_t lo, hi, processed, skipped; }; std::vector<Slice> slice(n_ivs, Slice{0, 0, 0, 0});
    mkp_stats acc; memset(&acc, 0, sizeof(acc));
    for (uint32_t i0 = 0; i0 < n_ivs;) {
      // a group: intervals i0 .. i1-1 follow each other on one contig with the same kind of focus (with partition keys every interval runs alone:
      // rows come grouped by key)
      uint32_t i1 = i0 + 1;
      while (c->partition_tags.empty() && i1 < n_ivs && ivs[i1].tid == ivs[i0].tid && ivs[i1].start == ivs[i1 - 1].end
          && (ivs[i1].focus != nullptr) == (ivs[i0].focus != nullptr) &&
             ivs[i1].combos == ivs[i0].combos && ivs[i1].n_combos == ivs[i0].n_combos && (uint64_t)ivs[i1].end - ivs[i0].start <= (1ull << 27)) i1++;
      mkp_shard sh = ivs[i0]; sh.end = ivs[i1 - 1].end;
      std::vector<uint8_t> focus;
      if (sh.focus && i1 > i0 + 1) { focus.resize((size_t)(sh.end - sh.start));
        for (uint32_t k = i0; k < i1; k++) memcpy(focus.data() + (ivs[k].start - sh.start), ivs[k].focus, (size_t)(ivs[k].end - ivs[k].start));
        sh.focus = focus.data(); }
      int rc = mkp_shard_begin(c, &sh); if (rc != MKP_OK) throw Error(rc, c->err);
      c->iv_starts.clear(); for (uint32_t k = i0; k < i1; k++) c->iv_starts.push_back(ivs[k].start);   // the duplicate-name rule is per interval
      // the group's records: its contig, starting before the window's end (the packer drops the other contigs itself; a record that ends
      // before the window only costs its packing)
      std::vector<mkp_record> mine; mine.reserve(n_recs);
      const int64_t hi = (int64_t)sh.end + MKP_HALO;
      for (uint32_t r = 0; r < n_recs; r++) if (recs[r].tid == sh.tid && (int64_t)recs[r].pos < hi) mine.push_back(recs[r]);
      rc = mkp_shard_add_records(c, mine.data(), (uint32_t)mine.size()); if (rc != MKP_OK) throw Error(rc, c->err);
      mkp_rows rows; memset(&rows, 0, sizeof(rows));
      rc = mkp_shard_run(c, &rows); if (rc != MKP_OK) throw Error(rc, c->err);
      // rows are in genome order (by key first with partition tags: then the group is one interval): cut at the interval ends
      const uint64_t base = c->batch_cols[0].size();
      const uint32_t* src[11] = {rows.pos, nullptr, rows.code_repr, rows.n_valid, rows.n_mod, rows.n_canonical, rows.n_other, rows.n_delete,
          rows.n_fail, rows.n_diff, rows.n_nocall};
      for (int k = 0; k < 11; k++) if (src[k]) c->batch_cols[k].insert(c->batch_cols[k].end(), src[k], src[k] + rows.n_rows);
      c->batch_strand.insert(c->batch_strand.end(), rows.strand, rows.strand + rows.n_rows);
        c->batch_motif.insert(c->batch_motif.end(), rows.motif_idx, rows.motif_idx + rows.n_rows);
      c->batch_key.insert(c->batch_key.end(), rows.partition_key, rows.partition_key + rows.n_rows);
      uint64_t at = 0;
      for (uint32_t k = i0; k < i1; k++) {
        uint64_t e = at; if (i1 == i0 + 1) e = rows.n_rows; else while (e < rows.n_rows && rows.pos[e] < ivs[k].end) e++;
        slice[k] = {base + at, base + e, k == i0 ? rows.processed_records : 0, k == i0 ? rows.skipped_records : 0}; at = e;
      }
      acc.pack_ms += c->stats.pack_ms; acc.h2d_ms += c->stats.h2d_ms; acc.kernel_ms += c->stats.kernel_ms; acc.d2h_ms += c->stats.d2h_ms;
        acc.n_rows += c->stats.n_rows; acc.n_reads += c->stats.n_reads;
      i0 = i1;
    }
    c->key_name_ptrs.clear(); for (auto& k : c->key_names) c->key_name_ptrs.push_back(k.c_str());
    for (uint32_t k = 0; k < n_ivs; k++) {
      mkp_rows& o = out[k]; memset(&o, 0, sizeof(o)); const Slice& sl = slice[k]; const uint64_t lo = sl.lo;
      o.n_rows = sl.hi - sl.lo; o.pos = c->batch_cols[0].data() + lo; o.strand = c->batch_strand.data() + lo;
        o.code_repr = c->batch_cols[2].data() + lo; o.motif_idx = c->batch_motif.data() + lo;
      o.n_valid = c->batch_cols[3].data() + lo; o.n_mod = c->batch_cols[4].data() + lo; o.n_canonical = c->batch_cols[5].data() + lo;
        o.n_other = c->batch_cols[6].data() + lo;
      o.n_delete = c->batch_cols[7].data() + lo; o.n_fail = c->batch_cols[8].data() + lo; o.n_diff = c->batch_cols[9].data() + lo;
        o.n_nocall = c->batch_cols[10].data() + lo;
      o.processed_records = sl.processed; o.skipped_records = sl.skipped;
      o.partition_key = c->batch_key.data() + lo; o.n_partition_keys = (uint32_t)c->key_name_ptrs.size();
        o.partition_key_names = c->key_name_ptrs.data();
    }
    // the batch's sums (the other fields: its last group)
    c->stats.pack_ms = acc.pack_ms; c->stats.h2d_ms = acc.h2d_ms; c->stats.kernel_ms = acc.kernel_ms; c->stats.d2h_ms = acc.d2h_ms;
  });
}

int mkp_hemi_shard_run(mkp_ctx* c, int32_t partner_offset, const uint32_t* interval_starts, uint32_t n_intervals, mkp_hemi_rows* out) {
  if (!c || (n_intervals && !interval_starts)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->shard_open) throw Error(MKP_E_INVALID, "mkp_shard_begin first");
    if (!c->caller_set) throw Error(MKP_E_INVALID, "mkp_set_caller first");
    if (partner_offset < -MKP_HALO || partner_offset > MKP_HALO) throw Error(MKP_E_UNSUPPORTED, "motif longer than the tile halo");
    std::vector<uint32_t> iv(interval_starts, interval_starts + n_intervals);
    if (iv.empty()) iv.push_back((uint32_t)std::max(c->shard.win_start, 0));
    const bool same = c->resident && c->resident_hemi && c->hemi_off == partner_offset && c->hemi_iv == iv;
    c->hemi = true; c->hemi_off = partner_offset;
    if (!same) { c->hemi_iv = std::move(iv); c->row_cap = 0; make_resident(c); }
    run_kernels(c, true);
    fetch_hemi_rows(c, out);
    c->stats.alg_bytes_decode += 8ull * c->stats.n_events;
    c->stats.alg_bytes_pileup += 8ull * c->stats.n_events + 44ull * c->stats.n_rows;
    c->stats.alg_bytes_rows = 0;
  });
}

int mkp_shard_rerun(mkp_ctx* c, uint32_t iters, mkp_rows* out) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->resident) throw Error(MKP_E_INVALID, "no resident shard: call mkp_shard_run once first");
    if (c->resident_hemi && out) throw Error(MKP_E_INVALID,
        "the resident shard ran as pileup-hemi: pass out = NULL here and read rows with mkp_hemi_shard_run");
    double d = 0, p = 0, g = 0;
    for (uint32_t i = 0; i < iters; i++) { run_kernels(c, true); d += c->stats.decode_kernel_ms; p += c->stats.pileup_kernel_ms;
      g += c->stats.gather_kernel_ms; }
    if (iters) { c->stats.decode_kernel_ms = d / iters; c->stats.pileup_kernel_ms = p / iters; c->stats.rows_kernel_ms = 0;
      c->stats.gather_kernel_ms = g / iters;
        c->stats.kernel_ms = (d + p + g) / iters; }
    if (out) fetch_rows(c, out);
  });
}

uint32_t mkp_abi_version(void) { return MKP_ABI_VERSION; }
size_t mkp_run_report_size(void) { return sizeof(mkp_run_report); }

int mkp_get_stats(const mkp_ctx* c, mkp_stats* out) { if (!c || !out) return MKP_E_INVALID; *out = c->stats; return MKP_OK; }
int mkp_shard_read_flags(const mkp_ctx* c, uint32_t* flags, uint32_t cap, uint32_t* n_reads) {
  if (!c || !n_reads || (cap && !flags)) return MKP_E_INVALID;
  const auto& hdr = c->shard.hdr;
  *n_reads = (uint32_t)hdr.size();
  for (size_t i = 0; i < hdr.size() && i < cap; i++) { const uint32_t f = hdr[i].flags;   // (the public bits are named, not the internal ones passed on)
    flags[i] = ((f & MKP_RF_REVERSE) ? MKP_READ_REVERSE : 0u) | ((f & MKP_RF_BAD) ? MKP_READ_TAG_ERROR : 0u) | ((f & MKP_RF_CIGW) ? MKP_READ_WIDE_CIGAR : 0u); }
  return MKP_OK;
}

int mkp_percentile(const float* xs, uint64_t n, float q, float* out) {  // percentile_linear_interp (thresholds.rs:17-38)
  if (!xs || !out || n < 2 || !(q >= 0.0f) || q > 1.0f) return MKP_E_THRESHOLD;
      // negative / NaN quantiles would index out of bounds (Rust's `as usize` saturates; here they are refused)
  if (q == 1.0f) { *out = xs[n - 1]; return MKP_OK; }
  float l = (float)(n - 1), lq = l * q, left = floorf(lq); uint64_t right = std::min<uint64_t>((uint64_t)ceilf(lq), n - 1);
  float g = lq - truncf(lq), a = xs[(uint64_t)left] * (1.0f - g), b = xs[right] * g;
  *out = a + b;
  return MKP_OK;
}

int mkp_bgzf_inflate(mkp_ctx* c, const uint8_t* bgzf, uint64_t n_bytes, const uint8_t** out, uint64_t* out_len, double* kernel_ms) {
  if (!c || (!bgzf && n_bytes) || !out || !out_len) return MKP_E_INVALID;
  return guarded(c, [&]() {
    std::vector<MkpBgzfBlock> blks; std::vector<uint32_t> crcs; uint64_t o = 0, total = 0;
    while (o < n_bytes) {   // header walk, as in load_bam (mkp_bam.hpp): gzip magic, FEXTRA with a BC subfield holding BSIZE
      if (o + 18 > n_bytes || bgzf[o] != 31 || bgzf[o + 1] != 139 || bgzf[o + 2] != 8 || !(bgzf[o + 3] & 4)) throw Error(MKP_E_IO, "not BGZF");
      uint16_t xlen; memcpy(&xlen, bgzf + o + 10, 2);
      uint64_t x = o + 12; const uint64_t xe = x + xlen; uint32_t bsize = 0; bool found = false;
      if (xe > n_bytes) throw Error(MKP_E_IO, "bad BGZF block");
      while (x + 4 <= xe) { uint16_t sl; memcpy(&sl, bgzf + x + 2, 2); if (bgzf[x] == 'B' && bgzf[x + 1] == 'C' && sl == 2 && x + 6 <= xe) {
          uint16_t b;
          memcpy(&b, bgzf + x + 4, 2); bsize = (uint32_t)b + 1; found = true; } x += 4 + (uint64_t)sl; }
      if (!found || o + bsize > n_bytes || bsize < (uint32_t)xlen + 20u) throw Error(MKP_E_IO, "bad BGZF block");
      uint32_t crc, isize; memcpy(&crc, bgzf + o + bsize - 8, 4); memcpy(&isize, bgzf + o + bsize - 4, 4);
      if (isize > 65536u) throw Error(MKP_E_IO, "BGZF block inflates to more than 64 KiB");
      blks.push_back({o + 12 + xlen, total, bsize - xlen - 20, isize}); crcs.push_back(crc);
      total += isize; o += bsize;
    }
    if (blks.size() > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "too many BGZF blocks");
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    c->d_zin.ensure(std::max<uint64_t>(n_bytes, 16)); c->d_zout.ensure(std::max<uint64_t>(total, 16));
      c->d_zblk.ensure(std::max<size_t>(blks.size(), 1) * sizeof(MkpBgzfBlock));
        c->d_zstat.ensure(std::max<size_t>(blks.size(), 1) * 4);
    h2d_copy(c->d_zin.p, bgzf, n_bytes);   // (caller memory and a temporary: through the library's page-locked staging, mkp_ctx.hpp)
    h2d_copy(c->d_zblk.p, blks.data(), blks.size() * sizeof(MkpBgzfBlock));
    hip_check(hipMemsetAsync(c->d_zstat.p, 0xff, std::max<size_t>(blks.size(), 1) * 4, c->stream), "memset");
    hip_check(hipEventRecord(c->ev[0], c->stream), "event");
    hip_check(mkp_launch_inflate_auto(c->stream, c->d_zin.as<uint8_t>(), c->d_zblk.as<MkpBgzfBlock>(), (uint32_t)blks.size(),
        c->d_zout.as<uint8_t>(), c->d_zstat.as<uint32_t>()), "inflate launch");
    hip_check(hipEventRecord(c->ev[1], c->stream), "event");
    std::vector<uint32_t> st(blks.size());
    c->h_inflated.resize(total);
    d2h_copy(st.data(), c->d_zstat.p, blks.size() * 4, c->stream);
    d2h_copy(c->h_inflated.data(), c->d_zout.p, total, c->stream);
    hip_check(hipStreamSynchronize(c->stream), "inflate sync");
    if (kernel_ms) { float ms = 0; hip_check(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]), "event"); *kernel_ms = ms; }
    std::atomic<long> bad{-1};
    host_parallel(blks.size(), 64, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) {
        const bool ok = st[i] == 0 && (uint32_t)crc32(crc32(0L, Z_NULL, 0), c->h_inflated.data() + blks[i].out_off, blks[i].out_len) == crcs[i];
        if (!ok) { long exp = -1; bad.compare_exchange_strong(exp, (long)i); }
      }
    });
    if (bad.load() >= 0) throw Error(MKP_E_IO,
        "corrupt BGZF data: block " + std::to_string(bad.load()) + " (decoder status " + std::to_string(st[(size_t)bad.load()]) + ")");
    *out = c->h_inflated.data(); *out_len = total;
  });
}

// ---- --device-inflate: the fetch path's inflate stage on the GPU (BamSource::dev_inflate).  Own stream and buffers: it runs on the
// prefetch thread while the shard in hand uses the context's stream.
struct PinnedBuf {   // page-locked host staging: pageable copies of a window's 270 MB ran at under 3 GB/s
  void* p = nullptr; size_t cap = 0;
  void ensure(size_t n) { if (n <= cap) return; release(); const size_t want = n + n / 8 + 4096;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr;
      throw Error(MKP_E_NOMEM, "hipHostMalloc failed"); } cap = want; }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
struct mkp_dev_inflater { int device = 0; hipStream_t stream = nullptr; DevBuf zin, zout, zblk, zstat; PinnedBuf pin_in, pin_out; std::mutex mu; };
}   // extern "C"
mkp_dev_inflater* mkp_internal_inflater_create(int device) {
  std::unique_ptr<mkp_dev_inflater> d(new mkp_dev_inflater()); d->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
  return d.release();
}
void mkp_internal_inflater_destroy(mkp_dev_inflater* d) {
  if (!d) return;
  (void)hipSetDevice(d->device); d->zin.release(); d->zout.release(); d->zblk.release(); d->zstat.release(); d->pin_in.release();
    d->pin_out.release();
  if (d->stream) (void)hipStreamDestroy(d->stream);
  delete d;
}
bool mkp_internal_device_inflate(void* user, const InflateJob& j) {
  mkp_dev_inflater* d = (mkp_dev_inflater*)user;
  if (!d || j.n_blks == 0 || j.n_blks > 0xffffffffull) return false;
  std::lock_guard<std::mutex> g(d->mu);
  try {
    auto ok = [](hipError_t e) { if (e != hipSuccess) throw Error(MKP_E_DEVICE, hipGetErrorString(e)); };
    ok(hipSetDevice(d->device));
    d->zin.ensure(j.comp_len + 16); d->zout.ensure(j.dtotal + 16); d->zblk.ensure(j.n_blks * sizeof(InflateBlk)); d->zstat.ensure(j.n_blks * 4);
    d->pin_in.ensure(j.comp_len + j.n_blks * sizeof(InflateBlk)); d->pin_out.ensure(j.dtotal + j.n_blks * 4);
    // file pages -> pinned (all cores, behind the foreground work), one H2D; inflate; one D2H into pinned; pinned -> the window's buffer
    uint8_t* pin = (uint8_t*)d->pin_in.p; const size_t piece = (size_t)4 << 20;
    HostPool::get().parallel((j.comp_len + piece - 1) / piece, [&](size_t i) { const size_t lo = i * piece, n = std::min(piece, j.comp_len - lo);
      memcpy(pin + lo, j.comp + lo, n); });
    memcpy(pin + j.comp_len, j.blks, j.n_blks * sizeof(InflateBlk));
    ok(hipMemcpyAsync(d->zin.p, pin, j.comp_len, hipMemcpyHostToDevice, d->stream));
    ok(hipMemcpyAsync(d->zblk.p, pin + j.comp_len, j.n_blks * sizeof(InflateBlk), hipMemcpyHostToDevice, d->stream));
    ok(hipMemsetAsync(d->zstat.p, 0xff, j.n_blks * 4, d->stream));
    ok(mkp_launch_inflate_auto(d->stream, d->zin.as<uint8_t>(), d->zblk.as<MkpBgzfBlock>(), (uint32_t)j.n_blks, d->zout.as<uint8_t>(),
        d->zstat.as<uint32_t>()));
    uint8_t* pout = (uint8_t*)d->pin_out.p;
    ok(hipMemcpyAsync(pout, d->zout.p, j.dtotal, hipMemcpyDeviceToHost, d->stream));
    ok(hipMemcpyAsync(pout + j.dtotal, d->zstat.p, j.n_blks * 4, hipMemcpyDeviceToHost, d->stream));
    ok(hipStreamSynchronize(d->stream));
    const uint32_t* st = (const uint32_t*)(pout + j.dtotal);   // (dtotal is a sum of block sizes; the status words may sit unaligned)
    // the host decoder takes the window and names the error
    for (size_t i = 0; i < j.n_blks; i++) { uint32_t v; memcpy(&v, (const uint8_t*)st + 4 * i, 4); if (v != 0) return false; }
    HostPool::get().parallel((j.dtotal + piece - 1) / piece, [&](size_t i) { const size_t lo = i * piece, n = std::min(piece, j.dtotal - lo);
      memcpy(j.dst + lo, pout + lo, n); });
    // the blocks' CRC32s (trailer word behind each payload), as the host decoder checks them: a mismatch hands the window to the host path,
    // which names the error
    std::atomic<bool> crc_bad{false};
    HostPool::get().parallel((j.n_blks + 63) / 64, [&](size_t g) { for (size_t i = g * 64; i < std::min(j.n_blks, (g + 1) * 64); i++) {
        const InflateBlk& b = j.blks[i];
        uint32_t want; memcpy(&want, j.comp + b.in_off + b.in_len, 4); if (crc32_of(j.dst + b.out_off, b.out_len) != want) crc_bad = true; } });
    if (crc_bad) return false;
    return true;
  } catch (const Error&) { return false; }
}
extern "C" {

int mkp_host_mm_ranks(const char* mm, uint32_t l_seq, uint32_t n_ml, mkp_host_tag* tags, uint32_t tags_cap, uint32_t* ranks, uint32_t ranks_cap) {
  if (!mm || (!tags && tags_cap) || (!ranks && ranks_cap)) return MKP_E_INVALID;
  try {
    // a synthetic one-record shard: qname "r", one M op, all-A SEQ, aux = MM:Z + ML:B:C (n_ml zero bytes)
    std::vector<uint8_t> data; data.push_back('r'); data.push_back(0);
    const uint32_t cg = (l_seq << 4) | 0u; data.insert(data.end(), (const uint8_t*)&cg, (const uint8_t*)&cg + 4);
    data.insert(data.end(), (l_seq + 1) / 2, 0x11); data.insert(data.end(), l_seq, 0xff);
    data.push_back('M'); data.push_back('M'); data.push_back('Z'); data.insert(data.end(), mm, mm + strlen(mm) + 1);
    data.push_back('M'); data.push_back('L'); data.push_back('B'); data.push_back('C');
      data.insert(data.end(), (const uint8_t*)&n_ml, (const uint8_t*)&n_ml + 4);
        data.insert(data.end(), n_ml, 0);
    mkp_record r; memset(&r, 0, sizeof(r)); r.tid = 0; r.pos = 0; r.l_qname = 2; r.n_cigar = 1; r.l_qseq = (int32_t)l_seq;
      r.l_data = (int32_t)data.size();
        r.data = data.data();
    Packer pk; ShardHost S; S.tid = 0; pk.add(r, S);
    if (S.hdr.empty() || (S.hdr[0].flags & MKP_RF_BAD)) return MKP_E_INVALID;
    const LayoutHost& L = pk.layouts[S.hdr[0].layout];
    if (L.tags.size() > tags_cap || S.ranks.size() > ranks_cap) return MKP_E_NOMEM;
    for (size_t t = 0; t < L.tags.size(); t++) {
      mkp_host_tag& o = tags[t]; memset(&o, 0, sizeof(o));
      o.base = L.tags[t].fb; o.negative_strand = L.tags[t].neg; o.mode = L.tags[t].mode; o.n_codes = (uint8_t)L.tags[t].codes.size();
      for (size_t i = 0; i < L.tags[t].codes.size() && i < 4; i++) o.codes[i] = L.tags[t].codes[i];
      o.rank_off = S.tagref[t].rank_off; o.n_ranks = S.tagref[t].n;
    }
    for (size_t i = 0; i < S.ranks.size(); i++) ranks[i] = S.ranks[i];
    return (int)L.tags.size();
  } catch (const Error& e) { return e.status; } catch (...) { return MKP_E_INVALID; }
}

int mkp_host_map_order(const uint32_t* code_reprs, uint32_t n, uint32_t* order_out) {
  if (!code_reprs || !order_out || n > 14) return MKP_E_INVALID;
  try { FxOrder m; for (uint32_t i = 0; i < n; i++) m.insert(code_reprs[i], (int)i); auto c = m.codes();
    for (size_t i = 0; i < c.size(); i++) order_out[i] = c[i];
      return (int)c.size(); }
  catch (...) { return MKP_E_INVALID; }
}

}  // extern "C"

// ---- threshold sampling on the device (decode kernels in sampling mode; the values stay in HBM)
// Decode `recs` in sampling mode.  n_vals[i] = number of argmax probabilities record i yields after the filters (0: rejected or
// nothing kept).  The values themselves stay on the device until mkp_internal_sample_take says which reads the schedule took.
namespace {
// the sampling pass over the packed reads of S (host-packed: everything goes up; resident: the arrays of the attached shard are in HBM
// already and S.hdr is the round's selection of its headers)
void sample_decode(mkp_ctx* c, ShardHost& S, bool resident, const uint8_t* bedmask, bool only_mapped, size_t n_expected,
    std::vector<uint32_t>* n_vals) {
  c->tables.build(c->packer.layouts, c->caller);
  MkpRunParams P; memset(&P, 0, sizeof(P));
  P.win_start = S.win_start; P.win_end = S.win_end; P.numeric_mode = c->caller.numeric_mode; P.edge_filter = c->caller.edge;
    P.edge_start = c->caller.edge_start;
  P.edge_end = c->caller.edge_end; P.edge_inverted = c->caller.edge_inverted; P.force_allow = 1;
    P.sample_mode = c->extract_mode ? 3 : c->summary_mode ? 2 : 1; P.only_mapped = only_mapped;
      P.has_focus = bedmask != nullptr;
  hip_check(hipSetDevice(c->device), "hipSetDevice");
  upload(c->d_hdr, S.hdr);
  if (!resident) { upload(c->d_cigar, S.cigar); upload(c->d_seq, S.seq); upload(c->d_tagref, S.tagref); upload(c->d_ranks, S.ranks);
    upload(c->d_ml, S.ml); }
  upload(c->d_layouts, c->tables.dev);
  { std::vector<uint32_t> ids; class_ids(S, c->tables, &ids, c->n_class, false); upload(c->d_read_ids, ids); }
  // the --include-bed mask of the contig: one upload per contig and sampling session, not per round (a 25 MB mask per round was most of
  // the 11.6 s a BED-filtered threshold estimate took on the C5 scale model); mkp_internal_bedmask_reset() starts a session
  const uint8_t* d_mask;
  if (bedmask) {
    const size_t len = (size_t)(S.win_end - S.win_start);
    if (bedmask != c->bedmask_src || len != c->bedmask_len) {
      c->d_bedmask.ensure(len); h2d_copy(c->d_bedmask.p, bedmask, len); c->bedmask_src = bedmask; c->bedmask_len = len;
    }
    d_mask = c->d_bedmask.as<uint8_t>();
  } else { c->d_focus.ensure(16); d_mask = c->d_focus.as<uint8_t>(); }
  const uint64_t cap = std::max<uint64_t>(S.n_events_cap, 1);
  c->d_events.ensure(cap * sizeof(MkpEvent)); c->d_vals.ensure(cap * sizeof(float));
    c->d_readout.ensure(std::max<size_t>(S.hdr.size(), 1) * sizeof(MkpReadOut));
      c->d_misc.ensure(64);
  uint32_t* words = c->d_misc.as<uint32_t>();   // a sampling pass's own pass words (mkp_launch.h): the error word is the one in use
  hip_check(hipMemsetAsync(words, 0, 16, c->stream), "memset");
  hip_check(mkp_launch_decode(c->stream, shard_arrays(c), c->d_read_ids.as<uint32_t>(), c->n_class, &P, words + MKP_PW_ERR, d_mask,
      c->d_vals.as<float>()), "decode(sample) launch");
  uint32_t h[4]; hip_check(hipMemcpyAsync(h, words, 16, hipMemcpyDeviceToHost, c->stream), "D2H");
  c->sample_ro.resize(S.hdr.size());
  if (!S.hdr.empty()) hip_check(hipMemcpyAsync(c->sample_ro.data(), c->d_readout.p, S.hdr.size() * sizeof(MkpReadOut), hipMemcpyDeviceToHost,
      c->stream), "D2H");
  hip_check(hipStreamSynchronize(c->stream), "sample sync");
  if (h[MKP_PW_ERR] & ERR_EVENT_CAP) throw Error(MKP_E_DEVICE, "internal: event segment overflow");
  if (S.hdr.size() != n_expected) throw Error(MKP_E_INVALID, "internal: sampler packed a different number of records");
  n_vals->resize(n_expected);
  for (size_t i = 0; i < n_expected; i++) (*n_vals)[i] = c->sample_ro[i].ok ? c->sample_ro[i].n_events : 0u;
  c->resident = false;
}
}  // namespace

int mkp_internal_sample(mkp_ctx* c, int32_t tid, uint32_t win_start, uint32_t win_end, const uint8_t* bedmask, const mkp_record* recs,
                        uint32_t n, bool only_mapped, std::vector<uint32_t>* n_vals) {
  if (!c || !n_vals) return MKP_E_INVALID;
  return guarded(c, [&]() {
    // a device-packed shard of an earlier run: its HBM arrays are about to be reused
    if (c->shard.dev_packed) { c->shard.clear(); c->shard_open = false; c->resident = false; }
    ShardHost& S = c->sample_shard; S.clear(); S.tid = tid; S.win_start = (int32_t)win_start; S.win_end = (int32_t)win_end;
    pack_records(c->packer, S, recs, n, [](const mkp_record&) { return true; });
    sample_decode(c, S, false, bedmask, only_mapped, n, n_vals);
  });
}

// The same pass over reads of the shard the device ingest attached (mkp_internal_shard_attach): `reads` index that shard's records; their
// CIGARs, bases and tags are in HBM already, only the round's headers (with their slices of the event buffer) go up.
int mkp_internal_sample_resident(mkp_ctx* c, uint32_t win_start, uint32_t win_end, const uint8_t* bedmask, const uint32_t* reads, uint32_t n,
    bool only_mapped, std::vector<uint32_t>* n_vals) {
  if (!c || !n_vals || (!reads && n)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    ShardHost& R = c->shard;
    if (!c->shard_open || !R.dev_packed) throw Error(MKP_E_INVALID, "internal: no device-packed shard attached");
    ShardHost& S = c->sample_shard; S.clear(); S.tid = R.tid; S.win_start = (int32_t)win_start; S.win_end = (int32_t)win_end; S.dev_packed = true;
    S.hdr.resize(n); uint64_t off = 0;
    for (uint32_t k = 0; k < n; k++) {
      if (reads[k] >= R.hdr.size() + R.so_hdr.size()) throw Error(MKP_E_INVALID, "internal: sampled read index out of range");
      MkpReadHdr h = reads[k] < R.hdr.size() ? R.hdr[reads[k]] : R.so_hdr[reads[k] - R.hdr.size()]; h.event_off = (uint32_t)off; off += h.event_cap;
      if (off > 0xfffffff0ull) throw Error(MKP_E_UNSUPPORTED, "sampling round exceeds 4 Gi call events");
      S.hdr[k] = h;
    }
    S.n_events_cap = off;
    S.tagref.swap(R.tagref);   // the headers' tag_off index the shard's tag table
    struct Back { ShardHost& a; ShardHost& b; ~Back() { a.tagref.swap(b.tagref); } } back{S, R};
    sample_decode(c, S, true, bedmask, only_mapped, n, n_vals);
  });
}

void mkp_internal_bedmask_reset(mkp_ctx* c) { if (c) { c->bedmask_src = nullptr; c->bedmask_len = 0; } }

int mkp_internal_set_extract(mkp_ctx* c, bool on) {
  if (!c) return MKP_E_INVALID;
  c->extract_mode = on; c->caller.read_base_caller = on; c->resident = false;
  return MKP_OK;
}

int mkp_internal_extract_fetch(mkp_ctx* c, std::vector<MkpEvent>* events, std::vector<float>* vals) {
  if (!c || !events || !vals) return MKP_E_INVALID;
  return guarded(c, [&]() {
    const uint64_t n = c->sample_shard.n_events_cap;
    events->resize(n); vals->resize(n);
    if (!n) return;
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    d2h_copy(events->data(), c->d_events.p, n * sizeof(MkpEvent), c->stream);
    d2h_copy(vals->data(), c->d_vals.p, n * sizeof(float), c->stream);
  });
}

// Add the values of the marked records of the last mkp_internal_sample batch to the resident sample and its level-0 histogram.
int mkp_internal_summary_begin(mkp_ctx* c) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() {
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    c->d_summary.ensure(134 * 8);
    hip_check(hipMemsetAsync(c->d_summary.p, 0, 134 * 8, c->stream), "memset");
    hip_check(hipStreamSynchronize(c->stream), "sync");
  });
}
int mkp_internal_summary_get(mkp_ctx* c, uint64_t out[134], std::vector<MkpSlot>* slots) {
  if (!c || !out || !slots) return MKP_E_INVALID;
  return guarded(c, [&]() {
    if (!c->d_summary.p) throw Error(MKP_E_INVALID, "internal: summary table not set up");
    hip_check(hipMemcpy(out, c->d_summary.p, 134 * 8, hipMemcpyDeviceToHost), "D2H");
    *slots = c->tables.st.slots;   // class 2 + s = Modified(slots[s].code_repr) on primary base slots[s].pb
  });
}
int mkp_internal_sample_take(mkp_ctx* c, const std::vector<uint8_t>& take) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() {
    const size_t n = c->sample_shard.hdr.size();
    if (take.size() != n) throw Error(MKP_E_INVALID, "internal: take mask size");
    uint64_t add = 0; for (size_t i = 0; i < n; i++) if (take[i] && c->sample_ro[i].ok) add += c->sample_ro[i].n_events;
    if (!add) return;
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    if (c->summary_mode) {   // `modkit summary`: count the taken reads' calls
      if (!c->d_summary.p) throw Error(MKP_E_INVALID, "internal: summary table not set up");
      c->d_take.ensure(std::max<size_t>(n, 16));
      hip_check(hipMemcpyAsync(c->d_take.p, take.data(), n, hipMemcpyHostToDevice, c->stream), "H2D");
      hip_check(mkp_launch_summary_accumulate(c->stream, shard_arrays(c), c->d_take.as<uint8_t>(), (uint32_t)n,
          c->d_summary.as<unsigned long long>(), c->d_summary.as<unsigned long long>() + 128), "summary accumulate launch");
      hip_check(hipStreamSynchronize(c->stream), "summary accumulate sync");
      return;
    }
    if (!c->d_hist0.p) { c->d_hist0.ensure(4 * 65536 * 4); c->d_hist1.ensure(65536 * 4); c->d_sample_cursor.ensure(16);
        hip_check(hipMemsetAsync(c->d_hist0.p, 0, 4 * 65536 * 4, c->stream), "memset");
          hip_check(hipMemsetAsync(c->d_sample_cursor.p, 0, 16, c->stream), "memset"); }
    const uint64_t need = c->sample_n + add;
    // the device histograms count in 32 bits: with 2^32 or more sampled values one bin could wrap (ML bytes put most values on a handful
    // of f32 patterns) — refused rather than estimated wrongly
    if (need > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED,
        "more than 2^32 - 1 sampled probabilities on one GPU (32-bit histogram counters); shard the estimate over more ranks");
    if (need * 4 > c->d_store.cap) {   // grow the resident sample, keeping what is there
      DevBuf nb; nb.ensure(std::max<uint64_t>(need * 4 * 2, 1u << 20));
      if (c->sample_n) hip_check(hipMemcpyAsync(nb.p, c->d_store.p, c->sample_n * 4, hipMemcpyDeviceToDevice, c->stream), "D2D");
      hip_check(hipStreamSynchronize(c->stream), "sync"); c->d_store.release(); c->d_store = nb; nb.p = nullptr; nb.cap = 0;
    }
    c->d_take.ensure(std::max<size_t>(n, 16));
    hip_check(hipMemcpyAsync(c->d_take.p, take.data(), n, hipMemcpyHostToDevice, c->stream), "H2D");
    hip_check(mkp_launch_sample_accumulate(c->stream, shard_arrays(c), c->d_take.as<uint8_t>(), (uint32_t)n, c->d_vals.as<float>(),
        c->d_store.as<uint32_t>(), c->d_store.cap / 4, c->d_sample_cursor.as<unsigned long long>(), c->d_hist0.as<uint32_t>(),
        c->d_misc.as<uint32_t>() + MKP_PW_ERR), "sample accumulate launch");
    hip_check(hipStreamSynchronize(c->stream), "sample accumulate sync");
    c->sample_n = need;
  });
}

namespace {
void require_sample(mkp_ctx* c) { if (!c->d_hist0.p) { hip_check(hipSetDevice(c->device), "hipSetDevice"); c->d_hist0.ensure(4 * 65536 * 4);
    c->d_hist1.ensure(65536 * 4);
    c->d_sample_cursor.ensure(16); hip_check(hipMemset(c->d_hist0.p, 0, 4 * 65536 * 4), "memset");
      hip_check(hipMemset(c->d_sample_cursor.p, 0, 16), "memset"); } }
}

extern "C" {

int mkp_histogram_begin(mkp_ctx* c) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() {
    require_sample(c);
    hip_check(hipMemset(c->d_hist0.p, 0, 4 * 65536 * 4), "memset"); hip_check(hipMemset(c->d_sample_cursor.p, 0, 16), "memset");
    c->sample_n = 0;
  });
}

int mkp_histogram_get(mkp_ctx* c, uint32_t base, uint32_t level, uint32_t prefix, uint64_t* out) {
  if (!c || !out || base > 3 || level > 1 || prefix > 0xffffu) return MKP_E_INVALID;
  return guarded(c, [&]() {
    require_sample(c);
    std::vector<uint32_t> h(65536);
    if (level == 0) hip_check(hipMemcpy(h.data(), c->d_hist0.as<uint32_t>() + (size_t)base * 65536, 65536 * 4, hipMemcpyDeviceToHost), "D2H");
    else {
      hip_check(hipMemsetAsync(c->d_hist1.p, 0, 65536 * 4, c->stream), "memset");
      hip_check(mkp_launch_sample_hist1(c->stream, c->d_store.as<uint32_t>(), c->sample_n, base, prefix, c->d_hist1.as<uint32_t>()), "hist1 launch");
      hip_check(hipMemcpyAsync(h.data(), c->d_hist1.p, 65536 * 4, hipMemcpyDeviceToHost, c->stream), "D2H");
      hip_check(hipStreamSynchronize(c->stream), "hist1 sync");
    }
    for (size_t i = 0; i < 65536; i++) out[i] = h[i];
  });
}

// The path's one collective behind the C ABI: the histogram is summed over the ranks of an RCCL communicator where it sits — widened to
// u64 in HBM, ncclAllReduce(ncclUint64, ncclSum) over xGMI on the context's stream, one D2H of the result.  librccl is looked up at
// run time (dlopen): a single-GPU build of the caller needs no RCCL.
}  // extern "C"
#include <dlfcn.h>
namespace {
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
// the HIP runtime this library is bound to (its device pointers mean something to that copy only): a process that also imports torch
// can hold a second copy of the ROCm libraries, with a librccl of its own next to it
std::string hip_runtime_path() { Dl_info i; if (dladdr((void*)&hipGetDeviceCount, &i) && i.dli_fname) return std::string(i.dli_fname);
  return std::string(); }
nccl_allreduce_fn rccl_allreduce() {
  static nccl_allreduce_fn fn = []() -> nccl_allreduce_fn {
    const char* forced = getenv("MKP_RCCL_LIB");   // (the library the caller made its communicator with)
    std::string beside = hip_runtime_path(); { const size_t sl = beside.rfind('/');
      beside = sl == std::string::npos ? std::string("librccl.so.1") : beside.substr(0, sl + 1) + "librccl.so.1"; }
    for (const char* name : {forced ? forced : beside.c_str(), beside.c_str(), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1",
        "/opt/rocm/lib/librccl.so"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) { if (void* f = dlsym(h, "ncclAllReduce")) return (nccl_allreduce_fn)f;
      } }
    return nullptr; }();
  return fn;
}
}  // namespace
extern "C" const char* mkp_internal_hip_runtime_path() { static const std::string p = hip_runtime_path(); return p.c_str(); }
extern "C" {
int mkp_histogram_allreduce(mkp_ctx* c, void* nccl_comm, uint32_t base, uint32_t level, uint32_t prefix, uint64_t* out) {
  if (!c || !nccl_comm || !out || base > 3 || level > 1 || prefix > 0xffffu) return MKP_E_INVALID;
  return guarded(c, [&]() {
    nccl_allreduce_fn ar = rccl_allreduce();
    if (!ar) throw Error(MKP_E_DEVICE, "librccl.so not found (ncclAllReduce)");
    require_sample(c);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    c->d_hist64.ensure(65536 * 8);
    const uint32_t* src = c->d_hist0.as<uint32_t>() + (size_t)base * 65536;
    if (level == 1) {
      hip_check(hipMemsetAsync(c->d_hist1.p, 0, 65536 * 4, c->stream), "memset");
      hip_check(mkp_launch_sample_hist1(c->stream, c->d_store.as<uint32_t>(), c->sample_n, base, prefix, c->d_hist1.as<uint32_t>()), "hist1 launch");
      src = c->d_hist1.as<uint32_t>();
    }
    hip_check(mkp_launch_widen(c->stream, src, c->d_hist64.as<unsigned long long>(), 65536u), "widen launch");
    const int rc = ar(c->d_hist64.p, c->d_hist64.p, 65536, /*ncclUint64*/ 5, /*ncclSum*/ 0, nccl_comm, c->stream);
    if (rc != 0) throw Error(MKP_E_DEVICE, "ncclAllReduce failed (" + std::to_string(rc) + ")");
    hip_check(hipMemcpyAsync(out, c->d_hist64.p, 65536 * 8, hipMemcpyDeviceToHost, c->stream), "D2H");
    hip_check(hipStreamSynchronize(c->stream), "all-reduce sync");
  });
}

// the same histograms over values the caller holds on the host (tests, and callers that sample elsewhere)
int mkp_histogram_from_values(const float* vals, uint64_t n, uint32_t level, uint32_t prefix, uint64_t* out) {
  if ((!vals && n) || !out || level > 1 || prefix > 0xffffu) return MKP_E_INVALID;
  memset(out, 0, 65536 * sizeof(uint64_t));
  for (uint64_t i = 0; i < n; i++) {
    uint32_t b; memcpy(&b, &vals[i], 4);
    if (b >> 30) return MKP_E_INVALID;   // probabilities are in [0, 2)
    if (level == 0) out[b >> 16]++; else if ((b >> 16) == prefix) out[b & 0xffffu]++;
  }
  return MKP_OK;
}

// percentile_linear_interp (thresholds.rs:17-38) needs xs[floor((n-1)q)] and xs[ceil((n-1)q)] of the sorted sample: which
// level-0 bins hold them, and at which rank inside the bin
int mkp_histogram_locate(const uint64_t* hist0, float q, uint32_t bins[2], uint64_t ranks_in_bin[2], uint64_t* n_out) {
  if (!hist0 || !bins || !ranks_in_bin) return MKP_E_INVALID;
  uint64_t n = 0; for (size_t i = 0; i < 65536; i++) n += hist0[i];
  if (n_out) *n_out = n;
  if (n < 2 || !(q >= 0.0f) || q > 1.0f) return MKP_E_THRESHOLD;
  uint64_t want[2];
  if (q == 1.0f) want[0] = want[1] = n - 1;
  else { const float l = (float)(n - 1), lq = l * q; want[0] = (uint64_t)floorf(lq); want[1] = (uint64_t)ceilf(lq);
    if (want[1] > n - 1) want[1] = n - 1;
      if (want[0] > n - 1) want[0] = n - 1; }
  for (int k = 0; k < 2; k++) {
    uint64_t cum = 0; bool found = false;
    for (uint32_t b = 0; b < 65536 && !found; b++) { if (want[k] < cum + hist0[b]) { bins[k] = b; ranks_in_bin[k] = want[k] - cum; found = true;
      } cum += hist0[b]; }
    if (!found) return MKP_E_THRESHOLD;
  }
  return MKP_OK;
}

int mkp_histogram_resolve(uint32_t prefix, const uint64_t* hist1, uint64_t rank_in_bin, float* value) {
  if (!hist1 || !value || prefix > 0xffffu) return MKP_E_INVALID;
  uint64_t cum = 0;
  for (uint32_t b = 0; b < 65536; b++) { if (rank_in_bin < cum + hist1[b]) { const uint32_t bits = (prefix << 16) | b; memcpy(value, &bits, 4);
      return MKP_OK;
      } cum += hist1[b]; }
  return MKP_E_THRESHOLD;
}

// the interpolation itself, on the two order statistics: y0 * (1 - g) + y1 * g with g = fract((n-1) q), in f32 as the reference does
int mkp_percentile_from_histogram(uint64_t n, float q, float y0, float y1, float* out) {
  if (!out || n < 2 || !(q >= 0.0f) || q > 1.0f) return MKP_E_THRESHOLD;
  if (q == 1.0f) { *out = y1; return MKP_OK; }
  const float l = (float)(n - 1), lq = l * q, g = lq - truncf(lq);
  *out = y0 * (1.0f - g) + y1 * g;
  return MKP_OK;
}

}  // extern "C"

// ---- sessions over bedMethyl rows that are already in HBM (mkp_ctx::RowTable): what region statistics and localize share
namespace {
// what the shared steps say about the feature they run for
struct RowTableWords { const char *begin, *needs, *launch, *inside, *holds; };
constexpr RowTableWords kStatsWords = {"mkp_stats_begin", "region statistics need", "region stats", "regions", "region statistics hold"};
constexpr RowTableWords kLocWords = {"mkp_localize_begin", "localize needs", "localize", "windows", "localize holds"};
constexpr RowTableWords kDmrWords = {"mkp_dmr_begin", "dmr pair needs", "dmr pair", "regions", "dmr pair holds"};
constexpr RowTableWords kDsitesWords = {"mkp_dmr_sites_begin", "dmr sites needs", "dmr sites", "tables", "dmr sites holds"};
constexpr RowTableWords kDrepsWords = {"mkp_dmr_reps_begin", "dmr replicates needs", "dmr replicates", "tables", "dmr replicates holds"};
constexpr RowTableWords kMergeWords = {"mkp_merge_begin", "bedmethyl merge needs", "bedmethyl merge", "tables", "bedmethyl merge holds"};
// the five columns the reducers read, on the device; info = 0 '+', 1 '-', 2 '.' in its low bits; rest = n_canonical, n_other, n_delete,
// n_fail, n_diff, n_nocall, which only the merge reads (not uploaded for the reducers)
struct RowCols { const uint32_t *pos, *info, *code, *n_valid, *n_mod; uint64_t n; const uint32_t* rest[6]; };

void rt_need_open(const mkp_ctx::RowTable& T, const RowTableWords& W) { if (!T.open) throw Error(MKP_E_INVALID, std::string(W.begin) + " first"); }

// a new session: tids = the contigs of the regions in device order (grouped by contig; < 0 = on none)
void rt_group_by_tid(mkp_ctx::RowTable& T, const std::vector<int32_t>& tids) {
  T.tid_range.clear(); T.tids_with_rows.clear(); T.most_per_tid = 0;
  for (uint32_t k = 0; k < tids.size(); k++) {
    if (tids[k] < 0) continue;
    auto it = T.tid_range.find(tids[k]);
    if (it == T.tid_range.end()) T.tid_range[tids[k]] = {k, k + 1}; else it->second.second = k + 1;
  }
  for (auto& kv : T.tid_range) T.most_per_tid = std::max(T.most_per_tid, kv.second.second - kv.second.first);
}

// the rows the last shard run left in HBM
RowCols rt_resident_rows(mkp_ctx* c, const mkp_ctx::RowTable& T, const RowTableWords& W) {
  rt_need_open(T, W);
  if (!c->partition_tags.empty()) throw Error(MKP_E_INVALID, std::string(W.needs)
      + " the rows in genome order: with partition tags set they come grouped by key");
  if (!c->resident || c->resident_hemi || c->hemi) throw Error(MKP_E_INVALID,
      "no pileup rows are resident: call mkp_shard_run first (pileup-hemi rows are pattern counts, not bedMethyl rows)");
  hip_check(hipSetDevice(c->device), "hipSetDevice");
  const MkpRowsDev& r = c->rows_dst;
  return {r.pos, r.info, r.code, r.n_valid, r.n_mod, c->stats.n_rows, {r.n_can, r.n_other, r.n_del, r.n_fail, r.n_diff, r.n_nocall}};
}

// the caller's rows, checked and uploaded into the session's own buffer (the first n_cols columns: the five the reducers read, with
// n_canonical the six of dmr, or all eleven; each padded to 64 rows)
RowCols rt_upload_rows(mkp_ctx* c, mkp_ctx::RowTable& T, const RowTableWords& W, const mkp_rows* rows, int n_cols = 5) {
  const bool all_columns = n_cols == 11;
  rt_need_open(T, W);
  const uint64_t n = rows->n_rows;
  if (n > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 rows in one call");
  if (n && (!rows->pos || !rows->strand || !rows->code_repr || !rows->n_valid || !rows->n_mod)) throw Error(MKP_E_INVALID,
      "pos, strand, code_repr, n_valid and n_mod are needed");
  if (n && n_cols == 6 && !rows->n_canonical) throw Error(MKP_E_INVALID, "n_canonical is needed as well");
  if (n && all_columns && (!rows->n_canonical || !rows->n_other || !rows->n_delete || !rows->n_fail || !rows->n_diff || !rows->n_nocall))
    throw Error(MKP_E_INVALID, "all eleven row columns are needed");
  std::vector<uint32_t> info(n);
  for (uint64_t i = 0; i < n; i++) {
    if (i && rows->pos[i] < rows->pos[i - 1]) throw Error(MKP_E_INVALID, "rows must be ascending in pos (row " + std::to_string(i) + ")");
    const uint8_t s = rows->strand[i];
    if (s != '+' && s != '-' && s != '.') throw Error(MKP_E_INVALID, "strand must be '+', '-' or '.' (row " + std::to_string(i) + ")");
    if (!rows->code_repr[i]) throw Error(MKP_E_INVALID, "0 is not a mod code (row " + std::to_string(i) + ")");
    info[i] = s == '+' ? 0u : s == '-' ? 1u : 2u;
  }
  hip_check(hipSetDevice(c->device), "hipSetDevice");
  hip_check(hipStreamSynchronize(c->stream), "sync");   // the previous call's kernels read the upload buffer
  const size_t col = ((size_t)n + 63) & ~(size_t)63;
  T.d_rows.ensure(std::max<size_t>(col, 64) * 4 * (size_t)n_cols);
  uint32_t* d = T.d_rows.as<uint32_t>();
  const uint32_t* src[11] = {rows->pos, info.data(), rows->code_repr, rows->n_valid, rows->n_mod, rows->n_canonical, rows->n_other,
      rows->n_delete, rows->n_fail, rows->n_diff, rows->n_nocall};
  for (int k = 0; k < n_cols; k++) h2d_copy(d + (size_t)k * col, src[k], (size_t)n * 4);
  RowCols r = {d, d + col, d + 2 * col, d + 3 * col, d + 4 * col, n, {}};
  for (int k = 0; k < 6; k++) r.rest[k] = 5 + k < n_cols ? d + (size_t)(5 + k) * col : nullptr;
  return r;
}

// launch(ev) queues the feature's kernels; with timing on it records three events around their two spans, which are waited for and summed
template <class Launch> void rt_timed(mkp_ctx::RowTable& T, const RowTableWords& W, Launch launch) {
  hip_check(launch(T.timing ? T.ev : nullptr), (std::string(W.launch) + " launch").c_str());
  if (T.timing) {
    hip_check(hipEventSynchronize(T.ev[2]), (std::string(W.launch) + " sync").c_str());
    float a = 0, b = 0; hip_check(hipEventElapsedTime(&a, T.ev[0], T.ev[1]), "event"); hip_check(hipEventElapsedTime(&b, T.ev[1], T.ev[2]), "event");
    T.kernel_ms[0] += a; T.kernel_ms[1] += b;
  }
}

// one piece of contig `tid`: launch(first, n, ev) runs the feature's kernels over its regions [first, first + n) of d_regions
template <class Launch> void rt_launch(mkp_ctx* c, mkp_ctx::RowTable& T, const RowTableWords& W, int32_t tid, uint64_t n_rows, Launch launch) {
  if (n_rows > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 rows in one piece");
  if (n_rows) T.tids_with_rows.insert(tid);
  auto it = T.tid_range.find(tid);
  if (!n_rows || it == T.tid_range.end()) return;
  rt_timed(T, W, [&](hipEvent_t* ev) { return launch(it->second.first, it->second.second - it->second.first, ev); });
}

int rt_timing(mkp_ctx* c, mkp_ctx::RowTable& T, int on, double ms_out[2]) {
  return guarded(c, [&]() {
    if (ms_out) { ms_out[0] = T.kernel_ms[0]; ms_out[1] = T.kernel_ms[1]; }
    if (on) for (auto& e : T.ev) if (!e) hip_check(hipEventCreate(&e), "hipEventCreate");
    T.timing = on != 0; if (on) T.kernel_ms[0] = T.kernel_ms[1] = 0;
  });
}

// misc = d_misc as read back: the slots' codes, then the error word
void rt_check_codes(const uint32_t* misc, const RowTableWords& W) {
  if (misc[MKP_STATS_MAX_CODES] & MKP_STATS_ERR_CODES) throw Error(MKP_E_UNSUPPORTED, std::string("the rows inside the ") + W.inside
      + " carry more than " + std::to_string(MKP_STATS_MAX_CODES) + " distinct mod codes: " + W.holds + " at most that many per run");
}
// the output columns (code, slot) for the slots in `mask`, by code
std::vector<std::pair<uint32_t, uint32_t>> rt_columns(const uint32_t* misc, uint32_t mask) {
  std::vector<std::pair<uint32_t, uint32_t>> cols;
  for (uint32_t s = 0; s < MKP_STATS_MAX_CODES; s++) if ((mask >> s) & 1u) cols.push_back({misc[s], s});
  std::sort(cols.begin(), cols.end());
  return cols;
}
}  // namespace

// ---- region statistics (`modkit stats`, include/mkpileup.h): the table stays in HBM between mkp_stats_begin and mkp_stats_get
namespace {
// d_misc: 16 slot codes, the error word, a pad word, the chunk total (u64)
constexpr size_t kStatsMiscBytes = 4 * MKP_STATS_MAX_CODES + 16;
void stats_launch(mkp_ctx* c, int32_t tid, const RowCols& r) {
  mkp_ctx::RegionStats& R = c->rstats;
  rt_launch(c, R, kStatsWords, tid, r.n, [&](uint32_t first, uint32_t n, hipEvent_t* ev) {
    uint32_t* misc = R.d_misc.as<uint32_t>();
    return mkp_launch_region_stats(c->stream, r.pos, r.info, r.code, r.n_valid, r.n_mod, (uint32_t)r.n, R.d_regions.as<MkpStatsRegion>() + first, n,
        R.d_lo.as<uint32_t>(), R.d_hi.as<uint32_t>(), R.d_cnt.as<uint32_t>(), R.d_off.as<unsigned long long>(),
        reinterpret_cast<unsigned long long*>(misc + MKP_STATS_MAX_CODES + 2), R.d_out.as<unsigned long long>(), R.d_seen.as<uint32_t>(), misc,
        misc + MKP_STATS_MAX_CODES, (unsigned long long)R.min_cov, R.fixed ? 1u : 0u, ev);
  });
}
}  // namespace

extern "C" {

int mkp_internal_stats_timing(mkp_ctx* c, int on, double ms_out[2]) { return c ? rt_timing(c, c->rstats, on, ms_out) : MKP_E_INVALID; }
int mkp_internal_skip_row_fetch(mkp_ctx* c, int on) { if (!c) return MKP_E_INVALID; c->skip_row_fetch = on != 0; return MKP_OK; }

int mkp_stats_begin(mkp_ctx* c, const mkp_region* regions, uint32_t n, const uint32_t* codes, uint32_t n_codes, uint64_t min_coverage) {
  if (!c || (!regions && n) || (!codes && n_codes)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::RegionStats& R = c->rstats;
    R.open = false;
    for (uint32_t i = 0; i < n; i++) {
      if (regions[i].start > regions[i].end) throw Error(MKP_E_INVALID, "region " + std::to_string(i) + ": start > end");
      if (regions[i].strand_rule < 1 || regions[i].strand_rule > 3) throw Error(MKP_E_INVALID, "region " + std::to_string(i)
          + ": strand_rule must be 1 ('+'), 2 ('-') or 3 (both)");
    }
    R.fixed_codes.assign(codes, codes + n_codes); std::sort(R.fixed_codes.begin(), R.fixed_codes.end());
    R.fixed_codes.erase(std::unique(R.fixed_codes.begin(), R.fixed_codes.end()), R.fixed_codes.end());
    for (uint32_t k : R.fixed_codes) if (!k) throw Error(MKP_E_INVALID, "0 is not a mod code");
    if (R.fixed_codes.size() > MKP_STATS_MAX_CODES) throw Error(MKP_E_UNSUPPORTED, "region statistics hold at most "
        + std::to_string(MKP_STATS_MAX_CODES) + " distinct mod codes per run");
    R.fixed = n_codes != 0; R.min_cov = min_coverage; R.n_regions = n;
    R.region_tid.resize(n);
    // the regions grouped by contig, caller order inside a contig; `out` = the caller's index
    std::vector<uint32_t> order(n); for (uint32_t i = 0; i < n; i++) { order[i] = i; R.region_tid[i] = regions[i].tid; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return regions[a].tid < regions[b].tid; });
    std::vector<MkpStatsRegion> dev(n); std::vector<int32_t> dev_tid(n);
    for (uint32_t k = 0; k < n; k++) { const mkp_region& g = regions[order[k]]; dev[k] = {g.start, g.end, g.strand_rule, order[k]}; dev_tid[k] = g.tid; }
    rt_group_by_tid(R, dev_tid);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(c->stream), "sync");   // (a previous session's kernels)
    const size_t n1 = std::max<size_t>(n, 1), m1 = std::max<size_t>(R.most_per_tid, 1);
    R.d_regions.ensure(n1 * sizeof(MkpStatsRegion)); R.d_out.ensure(n1 * 2 * MKP_STATS_MAX_CODES * 8); R.d_seen.ensure(n1 * 4);
    R.d_misc.ensure(kStatsMiscBytes); R.d_lo.ensure(m1 * 4); R.d_hi.ensure(m1 * 4); R.d_cnt.ensure(m1 * 4); R.d_off.ensure((m1 + 1) * 8);
    h2d_copy(R.d_regions.p, dev.data(), (size_t)n * sizeof(MkpStatsRegion));
    uint32_t misc[kStatsMiscBytes / 4] = {0}; for (size_t k = 0; k < R.fixed_codes.size(); k++) misc[k] = R.fixed_codes[k];
    h2d_copy(R.d_misc.p, misc, sizeof(misc));
    hip_check(hipMemsetAsync(R.d_out.p, 0, n1 * 2 * MKP_STATS_MAX_CODES * 8, c->stream), "memset");
    hip_check(hipMemsetAsync(R.d_seen.p, 0, n1 * 4, c->stream), "memset");
    hip_check(hipStreamSynchronize(c->stream), "sync");
    R.open = true;
  });
}

int mkp_stats_add_resident(mkp_ctx* c) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() { stats_launch(c, c->shard.tid, rt_resident_rows(c, c->rstats, kStatsWords)); });
}

int mkp_stats_add_rows(mkp_ctx* c, int32_t tid, const mkp_rows* rows) {
  if (!c || !rows) return MKP_E_INVALID;
  return guarded(c, [&]() { stats_launch(c, tid, rt_upload_rows(c, c->rstats, kStatsWords, rows)); });
}

int mkp_stats_get(mkp_ctx* c, mkp_stats_out* out) {
  if (!c || !out) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::RegionStats& R = c->rstats;
    rt_need_open(R, kStatsWords);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    uint32_t misc[kStatsMiscBytes / 4];
    d2h_copy(misc, R.d_misc.p, sizeof(misc), c->stream);
    rt_check_codes(misc, kStatsWords);
    const uint32_t n = R.n_regions;
    std::vector<uint64_t> tab((size_t)n * 2 * MKP_STATS_MAX_CODES); std::vector<uint32_t> seen(n);
    d2h_copy(tab.data(), R.d_out.p, tab.size() * 8, c->stream); d2h_copy(seen.data(), R.d_seen.p, (size_t)n * 4, c->stream);
    // columns: the given codes (slot = place in the sorted list), or the slots some region counted a row in, by code
    std::vector<std::pair<uint32_t, uint32_t>> cols;   // code, slot
    if (R.fixed) for (uint32_t k = 0; k < R.fixed_codes.size(); k++) cols.push_back({R.fixed_codes[k], k});
    else { uint32_t any = 0; for (uint32_t m : seen) any |= m;
      cols = rt_columns(misc, any); }
    const size_t nc = cols.size();
    R.h_codes.resize(nc); R.h_mod.assign((size_t)n * nc, 0); R.h_valid.assign((size_t)n * nc, 0); R.h_has.resize(n);
    for (size_t k = 0; k < nc; k++) R.h_codes[k] = cols[k].first;
    for (uint32_t r = 0; r < n; r++) {
      R.h_has[r] = R.tids_with_rows.count(R.region_tid[r]) && R.region_tid[r] >= 0 ? 1 : 0;
      for (size_t k = 0; k < nc; k++) { const uint64_t* e = &tab[((size_t)r * MKP_STATS_MAX_CODES + cols[k].second) * 2];
        R.h_mod[(size_t)r * nc + k] = e[0]; R.h_valid[(size_t)r * nc + k] = e[1]; }
    }
    out->n_regions = n; out->n_codes = (uint32_t)nc; out->code_repr = R.h_codes.data(); out->n_mod = R.h_mod.data();
    out->n_valid = R.h_valid.data(); out->contig_has_rows = R.h_has.data();
  });
}

}  // extern "C"

// ---- localize (`modkit localize`, include/mkpileup.h): the offset table stays in HBM between mkp_localize_begin and mkp_localize_get
namespace {
// d_misc: 16 slot codes, the error word, a pad word
constexpr size_t kLocMiscBytes = 4 * MKP_STATS_MAX_CODES + 8;
size_t loc_table_cells(uint32_t window) { return (size_t)MKP_STATS_MAX_CODES * (2 * (size_t)window + 1) * 3; }
void localize_launch(mkp_ctx* c, int32_t tid, const RowCols& r) {
  mkp_ctx::Localize& L = c->loc;
  rt_launch(c, L, kLocWords, tid, r.n, [&](uint32_t first, uint32_t n, hipEvent_t* ev) {
    uint32_t* misc = L.d_misc.as<uint32_t>();
    return mkp_launch_localize(c->stream, r.pos, r.info, r.code, r.n_valid, r.n_mod, (uint32_t)r.n, L.d_regions.as<MkpLocRegion>() + first, n,
        L.d_lo.as<uint32_t>(), L.d_hi.as<uint32_t>(), L.window, L.stranded, L.d_tab.as<unsigned long long>(), misc, misc + MKP_STATS_MAX_CODES, ev);
  });
}
}  // namespace

extern "C" {

int mkp_internal_localize_timing(mkp_ctx* c, int on, double ms_out[2]) { return c ? rt_timing(c, c->loc, on, ms_out) : MKP_E_INVALID; }

int mkp_localize_begin(mkp_ctx* c, const mkp_region* regions, uint32_t n, const uint64_t* contig_len_by_tid, uint32_t n_contigs, uint32_t window,
    int stranded, int stranded_features) {
  if (!c || (!regions && n) || (!contig_len_by_tid && n_contigs)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Localize& L = c->loc;
    L.open = false;
    if (window > MKP_LOC_MAX_WINDOW) throw Error(MKP_E_UNSUPPORTED, "localize: a window of more than " + std::to_string(MKP_LOC_MAX_WINDOW)
        + " offsets to either side is not supported");
    if (stranded < 0 || stranded > 2) throw Error(MKP_E_INVALID, "stranded must be 0 (none), 1 (same) or 2 (opposite)");
    if (stranded_features < 0 || stranded_features > 3) throw Error(MKP_E_INVALID,
        "stranded_features must be 0 (the region's own strand), 1 ('+'), 2 ('-') or 3 ('.')");
    for (uint32_t k = 0; k < n_contigs; k++) if (contig_len_by_tid[k] > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED,
        "contig " + std::to_string(k) + " is longer than 2^32 - 1");
    // load_focus_regions (subcommand.rs:163-187) on the regions whose contig is in the sizes table, then grouped by contig
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < n; i++) {
      if (regions[i].strand_rule < 1 || regions[i].strand_rule > 3) throw Error(MKP_E_INVALID, "region " + std::to_string(i)
          + ": strand_rule must be 1 ('+'), 2 ('-') or 3 (both)");
      if (regions[i].tid >= 0 && (uint32_t)regions[i].tid < n_contigs) order.push_back(i);
    }
    if (order.empty()) throw Error(MKP_E_INVALID, "failed to find any valid regions: none lies on a contig of the sizes table");
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return regions[a].tid < regions[b].tid; });
    const uint64_t w = window;
    std::vector<MkpLocRegion> dev(order.size());
    L.kept_tid.resize(order.size());
    for (uint32_t k = 0; k < order.size(); k++) {
      const mkp_region& g = regions[order[k]];
      const uint64_t mp = ((uint64_t)g.start + (uint64_t)g.end) / 2;
      const uint64_t ws = mp >= w + 1 ? mp - (w + 1) : 0, we = std::min(mp + w, contig_len_by_tid[g.tid]);
      const uint64_t anchor = (ws + we) / 2;
      // every row of a non-empty window has its offset anchor - pos in [-window, window]: the table's 2 window + 1 cells hold them all
      if (we > ws && (anchor - ws > w || (we - 1) - std::min(anchor, we - 1) > w)) throw Error(MKP_E_INVALID, "region " + std::to_string(order[k])
          + ": an offset beyond the window");
      const uint32_t fetch = stranded_features ? (uint32_t)stranded_features : (uint32_t)g.strand_rule;
      dev[k] = {(uint32_t)ws, (uint32_t)we, (uint32_t)anchor, fetch | ((uint32_t)g.strand_rule << 8)};
      L.kept_tid[k] = g.tid;
    }
    rt_group_by_tid(L, L.kept_tid);
    L.window = window; L.stranded = (uint32_t)stranded;
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(c->stream), "sync");   // (a previous session's kernels)
    const size_t m1 = std::max<size_t>(L.most_per_tid, 1);
    L.d_regions.ensure(dev.size() * sizeof(MkpLocRegion)); L.d_tab.ensure(loc_table_cells(window) * 8); L.d_misc.ensure(kLocMiscBytes);
    L.d_lo.ensure(m1 * 4); L.d_hi.ensure(m1 * 4);
    h2d_copy(L.d_regions.p, dev.data(), dev.size() * sizeof(MkpLocRegion));
    hip_check(hipMemsetAsync(L.d_misc.p, 0, kLocMiscBytes, c->stream), "memset");
    hip_check(hipMemsetAsync(L.d_tab.p, 0, loc_table_cells(window) * 8, c->stream), "memset");
    hip_check(hipStreamSynchronize(c->stream), "sync");
    L.open = true;
  });
}

int mkp_localize_add_resident(mkp_ctx* c) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() { localize_launch(c, c->shard.tid, rt_resident_rows(c, c->loc, kLocWords)); });
}

int mkp_localize_add_rows(mkp_ctx* c, int32_t tid, const mkp_rows* rows) {
  if (!c || !rows) return MKP_E_INVALID;
  return guarded(c, [&]() { localize_launch(c, tid, rt_upload_rows(c, c->loc, kLocWords, rows)); });
}

int mkp_localize_get(mkp_ctx* c, mkp_localize_out* out) {
  if (!c || !out) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Localize& L = c->loc;
    rt_need_open(L, kLocWords);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    uint32_t misc[kLocMiscBytes / 4];
    d2h_copy(misc, L.d_misc.p, sizeof(misc), c->stream);
    rt_check_codes(misc, kLocWords);
    bool any_region = false;
    for (int32_t tid : L.kept_tid) if (L.tids_with_rows.count(tid)) { any_region = true; break; }
    if (!any_region) throw Error(MKP_E_INVALID, "failed to find any valid regions: no row was added on a contig that has one");
    const size_t n_off = 2 * (size_t)L.window + 1;
    std::vector<uint64_t> tab(loc_table_cells(L.window));
    d2h_copy(tab.data(), L.d_tab.p, tab.size() * 8, c->stream);
    // columns: the slots with a counted row in some cell, by code
    uint32_t counted = 0;
    for (uint32_t s = 0; s < MKP_STATS_MAX_CODES; s++) {
      if (!misc[s]) continue;
      bool any = false; for (size_t o = 0; o < n_off && !any; o++) any = tab[((size_t)s * n_off + o) * 3 + 2] != 0;
      if (any) counted |= 1u << s;
    }
    const std::vector<std::pair<uint32_t, uint32_t>> cols = rt_columns(misc, counted);   // code, slot
    const size_t nc = cols.size();
    L.h_codes.resize(nc); L.h_mod.resize(nc * n_off); L.h_valid.resize(nc * n_off); L.h_rows.resize(nc * n_off);
    for (size_t k = 0; k < nc; k++) { L.h_codes[k] = cols[k].first;
      for (size_t o = 0; o < n_off; o++) { const uint64_t* e = &tab[((size_t)cols[k].second * n_off + o) * 3];
        // the table's index is anchor + window - pos = offset + window already
        L.h_mod[k * n_off + o] = e[0]; L.h_valid[k * n_off + o] = e[1]; L.h_rows[k * n_off + o] = e[2]; } }
    out->n_codes = (uint32_t)nc; out->window = L.window; out->code_repr = L.h_codes.data(); out->n_mod = L.h_mod.data();
    out->n_valid = L.h_valid.data(); out->n_rows = L.h_rows.data();
  });
}

}  // extern "C"

// ---- bedmethyl merge (`modkit bedmethyl merge`, include/mkpileup.h): one merged row table per contig stays in HBM between mkp_merge_begin
// and the mkp_merge_get calls; every add is one two-way merge (mkp_merge.hip)
namespace {
// d_misc: rows of the new table, the error word (kept over the session), the rows below the contig's length, a pad word
constexpr size_t kMergeMiscBytes = 16;
MkpRowsDev rows_at(uint32_t* p, uint64_t stride) {
  return {p, p + stride, p + 2 * stride, p + 3 * stride, p + 4 * stride, p + 5 * stride, p + 6 * stride, p + 7 * stride, p + 8 * stride,
      p + 9 * stride, p + 10 * stride};
}
// r: rows of contig `tid` on the device, ascending pos; those at pos >= the contig's length (n_kept on) are dropped and counted
void merge_add(mkp_ctx* c, int32_t tid, const RowCols& r, uint64_t n_kept) {
  mkp_ctx::Merge& M = c->merge;
  if (r.n > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 rows in one piece");
  M.n_dropped += r.n - n_kept;
  if (!n_kept) return;
  mkp_ctx::Merge::Contig& C = M.contigs[tid];
  const uint64_t total = (uint64_t)C.n + n_kept;
  if (total > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 rows on one contig");
  const int to = C.cur ^ 1;
  const uint64_t stride = (total + 63) & ~(uint64_t)63;
  C.buf[to].ensure(stride * 44); C.stride[to] = stride;
  M.d_stage.ensure(stride * 44);
  const size_t n_tiles = mkp_merge_tiles(total);
  M.d_cuts.ensure((n_tiles + 1) * sizeof(MkpMergeCut)); M.d_counts.ensure(n_tiles * 4); M.d_offsets.ensure(n_tiles * 4);
  const MkpRowsDev a = rows_at(C.buf[C.cur].as<uint32_t>(), C.stride[C.cur]), out = rows_at(C.buf[to].as<uint32_t>(), stride),
      stage = rows_at(M.d_stage.as<uint32_t>(), stride);
  const MkpRowsDev b = {const_cast<uint32_t*>(r.pos), const_cast<uint32_t*>(r.info), const_cast<uint32_t*>(r.code), const_cast<uint32_t*>(r.n_valid),
      const_cast<uint32_t*>(r.n_mod), const_cast<uint32_t*>(r.rest[0]), const_cast<uint32_t*>(r.rest[1]), const_cast<uint32_t*>(r.rest[2]),
      const_cast<uint32_t*>(r.rest[3]), const_cast<uint32_t*>(r.rest[4]), const_cast<uint32_t*>(r.rest[5])};
  uint32_t* misc = M.d_misc.as<uint32_t>();
  rt_timed(M, kMergeWords, [&](hipEvent_t* ev) {
    return mkp_launch_merge(c->stream, &a, C.n, &b, (uint32_t)n_kept, &stage, &out, M.d_cuts.as<MkpMergeCut>(), M.d_counts.as<uint32_t>(),
        M.d_offsets.as<uint32_t>(), misc, misc + 1, ev);
  });
  // the one round trip of an add: the new table's size (the next add's buffers are sized by it) and the error word
  uint32_t words[2] = {0, 0};
  d2h_copy(words, misc, sizeof(words), c->stream);
  M.err_bits |= words[1];
  if (words[1] & MKP_MERGE_ERR_TILE) throw Error(MKP_E_UNSUPPORTED, "bedmethyl merge: one position of contig " + std::to_string(tid)
      + " holds more than " + std::to_string(MKP_MERGE_CAP - MKP_MERGE_TILE) + " rows: more than a tile of the merge kernel has room for");
  C.n = words[0]; C.cur = to;
}
uint64_t merge_contig_len(const mkp_ctx::Merge& M, int32_t tid) { return tid >= 0 && (size_t)tid < M.contig_len.size() ? M.contig_len[(size_t)tid] : 0ull; }
}  // namespace

extern "C" {

int mkp_internal_merge_timing(mkp_ctx* c, int on, double ms_out[2]) { return c ? rt_timing(c, c->merge, on, ms_out) : MKP_E_INVALID; }

int mkp_merge_begin(mkp_ctx* c, const uint64_t* contig_len_by_tid, uint32_t n_contigs) {
  if (!c || (!contig_len_by_tid && n_contigs)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Merge& M = c->merge;
    M.open = false;
    for (uint32_t k = 0; k < n_contigs; k++) if (contig_len_by_tid[k] > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED,
        "contig " + std::to_string(k) + " is longer than 2^32 - 1");
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(c->stream), "sync");   // (a previous session's kernels)
    for (auto& kv : M.contigs) for (DevBuf& b : kv.second.buf) b.release();
    M.contigs.clear(); M.contig_len.assign(contig_len_by_tid, contig_len_by_tid + n_contigs); M.n_dropped = 0; M.err_bits = 0;
    M.d_misc.ensure(kMergeMiscBytes);
    hip_check(hipMemsetAsync(M.d_misc.p, 0, kMergeMiscBytes, c->stream), "memset");
    hip_check(hipStreamSynchronize(c->stream), "sync");
    M.open = true;
  });
}

int mkp_merge_add_resident(mkp_ctx* c) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Merge& M = c->merge;
    const RowCols r = rt_resident_rows(c, M, kMergeWords);
    if (r.n > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 rows in one piece");
    const uint64_t len = merge_contig_len(M, c->shard.tid);
    uint64_t n_kept = r.n;
    if (!len) n_kept = 0;
    else if (r.n && (int64_t)c->shard.win_end > (int64_t)len) {   // the shard's window reaches beyond the sizes' length: count the rows in front of it
      uint32_t* misc = M.d_misc.as<uint32_t>();
      hip_check(mkp_launch_merge_rows_below(c->stream, r.pos, (uint32_t)r.n, (uint32_t)len, misc + 2), "bedmethyl merge launch");
      uint32_t below = 0; d2h_copy(&below, misc + 2, 4, c->stream); n_kept = below;
    }
    merge_add(c, c->shard.tid, r, n_kept);
  });
}

int mkp_merge_add_rows(mkp_ctx* c, int32_t tid, const mkp_rows* rows) {
  if (!c || !rows) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Merge& M = c->merge;
    const RowCols r = rt_upload_rows(c, M, kMergeWords, rows, 11);
    const uint64_t len = merge_contig_len(M, tid);
    const uint64_t n_kept = len > 0xffffffffull ? r.n : (uint64_t)(std::lower_bound(rows->pos, rows->pos + r.n, (uint32_t)len) - rows->pos);
    merge_add(c, tid, r, n_kept);
  });
}

int mkp_merge_get(mkp_ctx* c, int32_t tid, mkp_rows* out, uint64_t* n_dropped) {
  if (!c || !out) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Merge& M = c->merge;
    rt_need_open(M, kMergeWords);
    if (M.err_bits & MKP_MERGE_ERR_TILE) throw Error(MKP_E_UNSUPPORTED, "bedmethyl merge: a position held more rows than a tile of the merge kernel has room for");
    if (M.err_bits & MKP_MERGE_ERR_SUM) throw Error(MKP_E_UNSUPPORTED,
        "bedmethyl merge: a summed count does not fit in 32 bits (rows carry 32-bit counts; the reference sums in 64 bits)");
    memset(out, 0, sizeof(*out));
    if (n_dropped) *n_dropped = M.n_dropped;
    auto it = M.contigs.find(tid);
    if (it == M.contigs.end() || !it->second.n) return;
    mkp_ctx::Merge::Contig& C = it->second;
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    const uint32_t* d = C.buf[C.cur].as<uint32_t>();
    for (int k = 0; k < 11; k++) { C.h_col[k].resize(C.n); d2h_copy(C.h_col[k].data(), d + (size_t)k * C.stride[C.cur], (size_t)C.n * 4, c->stream); }
    C.h_strand.resize(C.n); C.h_motif.assign(C.n, -1);
    for (uint32_t i = 0; i < C.n; i++) C.h_strand[i] = (uint8_t)"+-."[C.h_col[1][i] & 3u];
    out->n_rows = C.n; out->pos = C.h_col[0].data(); out->strand = C.h_strand.data(); out->code_repr = C.h_col[2].data();
    out->motif_idx = C.h_motif.data(); out->n_valid = C.h_col[3].data(); out->n_mod = C.h_col[4].data(); out->n_canonical = C.h_col[5].data();
    out->n_other = C.h_col[6].data(); out->n_delete = C.h_col[7].data(); out->n_fail = C.h_col[8].data(); out->n_diff = C.h_col[9].data();
    out->n_nocall = C.h_col[10].data();
  });
}

}  // extern "C"

// ---- the device bedMethyl reader (mkp_bedmethyl.hip; mkp_merge_add_file and mkp_bedmethyl_read_device of include/mkpileup.h): a plain or
// BGZF bedMethyl file becomes row columns in HBM piece by piece; compressed blocks (or the plain bytes) go up, the text and the rows stay there
namespace {

struct PinnedFile {   // the whole file in page-locked memory (16 readable bytes behind it)
  uint8_t* p = nullptr; size_t n = 0;
  ~PinnedFile() { if (p) (void)hipHostFree(p); }
  void read(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw Error(MKP_E_IO, "failed to open bedMethyl " + path);
    struct Close { FILE* f; ~Close() { fclose(f); } } close{f};
    if (fseeko(f, 0, SEEK_END) != 0) throw Error(MKP_E_IO, "failed to read bedMethyl " + path);
    const off_t size = ftello(f);
    if (size < 0 || fseeko(f, 0, SEEK_SET) != 0) throw Error(MKP_E_IO, "failed to read bedMethyl " + path);
    if (hipHostMalloc(reinterpret_cast<void**>(&p), (size_t)size + 16, hipHostMallocDefault) != hipSuccess) { p = nullptr;
      throw Error(MKP_E_NOMEM, "hipHostMalloc of " + std::to_string((size_t)size + 16) + " bytes for " + path + " failed"); }
    while (n < (size_t)size) { const size_t got = fread(p + n, 1, (size_t)size - n, f); if (!got) break; n += got; }
    if (n != (size_t)size) throw Error(MKP_E_IO, "failed to read bedMethyl " + path);
    memset(p + n, 0, 16);
  }
};

// MKP_BEDMETHYL_PIECE_KB: the text a piece holds at most (KiB; default 131072 = the ingest's 128 MiB stages; 64 .. 1048576)
uint64_t bedin_piece_bytes() {
  uint64_t kb = 131072;
  if (const char* e = getenv("MKP_BEDMETHYL_PIECE_KB")) { char* end = nullptr; const unsigned long long v = strtoull(e, &end, 10);
    if (end != e && *end == 0) kb = v; }
  return std::min<uint64_t>(std::max<uint64_t>(kb, 64), 1048576) * 1024;
}

// What the device found in a piece, said by the host reader: text[0, limit) of the piece comes back and is read again.  A line that does not
// parse throws the host reader's own message (line numbers count on from line_base); then a line too long for a piece, then a pos that
// descends inside a contig run (across the seam too: last_chrom / last_pos, the row in front of the piece).  Nothing found: the two readers disagree.
[[noreturn]] void bedin_fail(mkp_ctx* c, const uint8_t* d_text, uint32_t limit, uint64_t line_base, const std::string& path, uint32_t bits,
    uint64_t err_off, uint64_t max_line, const std::string* last_chrom, uint32_t last_pos) {
  std::vector<uint8_t> text(limit);
  d2h_copy(text.data(), d_text, limit, c->stream);
  mkp_bedmethyl_file f; std::vector<uint64_t> line_nos;
  parse_bedmethyl_text(text.data(), text.size(), path, line_base, f, &line_nos);
  if (bits & MKP_BEDIN_ERR_LONG) {
    uint64_t line_no = line_base;
    for (size_t p = 0; p < text.size();) { const uint8_t* nl = (const uint8_t*)memchr(text.data() + p, '\n', text.size() - p);
      const size_t e = nl ? (size_t)(nl - text.data()) : text.size(); line_no++;
      if (e - p > max_line && text[p] != '#') throw Error(MKP_E_UNSUPPORTED, "line " + std::to_string(line_no) + " of " + path + " is longer than "
          + std::to_string(max_line) + " bytes: it does not fit a piece of the device reader (MKP_BEDMETHYL_PIECE_KB)");
      p = e + 1; }
  }
  for (size_t k = 0; k < f.runs.size(); k++) {
    const mkp_bedmethyl_file::Run& u = f.runs[k];
    const bool goes_on = k == 0 && last_chrom && *last_chrom == u.chrom;
    for (uint64_t i = u.first; i < u.first + u.n; i++) {
      const bool first = i == u.first;
      if (first && !goes_on) continue;
      if (f.col[0][i] < (first ? last_pos : f.col[0][i - 1])) throw Error(MKP_E_INVALID, "line " + std::to_string(line_nos[i]) + " of " + path
          + ": rows must be ascending in pos inside a run of lines on one contig (" + std::to_string(f.col[0][i]) + " follows "
          + std::to_string(first ? last_pos : f.col[0][i - 1]) + " on " + u.chrom + ")");
    }
  }
  throw Error(MKP_E_DEVICE, "device and host readers disagree on " + path + ": the device reader reports error bits " + std::to_string(bits)
      + " at byte " + std::to_string(err_off) + " of the piece behind line " + std::to_string(line_base) + ", the host reader finds nothing wrong there");
}

float bedin_elapsed(hipEvent_t a, hipEvent_t b) { float ms = 0; hip_check(hipEventElapsedTime(&ms, a, b), "event"); return ms; }

// The file at `path` through the device reader.  sink(chrom, rows, goes_on) takes every contig run of every piece in file order, its rows
// on the device (the next piece overwrites them: sink is done with them when it returns); goes_on: the run continues the one handed over
// last (a run cut by a piece seam).
template <class Sink> void bedin_read_file(mkp_ctx* c, const std::string& path, Sink sink) {
  mkp_ctx::BedIn& B = c->bedin;
  hip_check(hipSetDevice(c->device), "hipSetDevice");
  for (auto& e : B.ev) if (!e) hip_check(hipEventCreate(&e), "hipEventCreate");
  auto t_read = std::chrono::steady_clock::now();
  PinnedFile file; file.read(path);
  const bool gz = is_gzip(file.p, file.n);
  std::vector<BgzfBlk> blks; if (gz) blks = bgzf_walk(file.p, file.n, path);
  uint64_t text_total = file.n;
  if (gz) { text_total = 0; for (const BgzfBlk& b : blks) text_total += b.isize; }
  B.ms[0] += ms_since(t_read);
  const uint64_t P = bedin_piece_bytes(), max_line = P - 1;
  // a BGZF piece takes whole blocks, at least one: up to 64 KiB more than P
  const size_t text_cap = (size_t)(((std::min(P, text_total) + 65536u + MKP_BEDIN_CHUNK - 1) / MKP_BEDIN_CHUNK + 1) * MKP_BEDIN_CHUNK);
  B.d_words.ensure(MKP_BEDIN_WORDS * 4);
  uint32_t* words = B.d_words.as<uint32_t>();
  auto too_long = [&](uint64_t line_base) { return Error(MKP_E_UNSUPPORTED, "line " + std::to_string(line_base + 1) + " of " + path + " is longer than "
      + std::to_string(max_line) + " bytes: it does not fit a piece of the device reader (MKP_BEDMETHYL_PIECE_KB)"); };
  // an empty block is checked here and never handed to the inflate kernel
  auto skip_empty = [&](size_t& bi) { while (bi < blks.size() && !blks[bi].isize) { bgzf_inflate_block_host(file.p, blks[bi], bi, nullptr, path); bi++; } };

  uint64_t pos = 0, line_base = 0; size_t bi = 0; uint32_t carry = 0; int cur = 0;
  bool have_last = false; std::string last_chrom; uint32_t last_pos = 0;
  skip_empty(bi);
  for (bool final_piece = gz ? bi == blks.size() : file.n == 0; !final_piece || carry;) {
    hip_check(hipStreamSynchronize(c->stream), "sync");   // the last piece's rows and text are done with
    B.d_text[cur].ensure(text_cap);
    uint8_t* text = B.d_text[cur].as<uint8_t>();
    uint32_t n = carry; std::vector<MkpBgzfBlock> dev_blks; std::vector<size_t> blk_index; uint64_t z_lo = 0, z_hi = 0;
    if (!gz) {
      if (carry >= P) throw too_long(line_base);
      const uint64_t take = std::min<uint64_t>(P - carry, file.n - pos);
      hip_check(hipEventRecord(B.ev[0], c->stream), "event");
      if (take) hip_check(hipMemcpyAsync(text + carry, file.p + pos, take, hipMemcpyHostToDevice, c->stream), "H2D");
      hip_check(hipEventRecord(B.ev[1], c->stream), "event");
      pos += take; n += (uint32_t)take; final_piece = pos == file.n;
    } else {
      if (carry > P) throw too_long(line_base);
      z_lo = bi < blks.size() ? blks[bi].start : 0; z_hi = z_lo;
      while (bi < blks.size() && (dev_blks.empty() || (uint64_t)n + blks[bi].isize <= P)) {
        const BgzfBlk& b = blks[bi];
        dev_blks.push_back({b.in_off - z_lo, (unsigned long long)n, b.in_len, b.isize}); blk_index.push_back(bi);
        n += b.isize; z_hi = b.start + b.bsize; bi++;
        skip_empty(bi);
      }
      final_piece = bi == blks.size();
      if (!dev_blks.empty()) {
        B.d_zin.ensure((size_t)(z_hi - z_lo) + 16); B.d_blk.ensure(dev_blks.size() * sizeof(MkpBgzfBlock)); B.d_stat.ensure(dev_blks.size() * 4);
        h2d_copy(B.d_blk.p, dev_blks.data(), dev_blks.size() * sizeof(MkpBgzfBlock));
      }
      hip_check(hipEventRecord(B.ev[0], c->stream), "event");
      if (!dev_blks.empty()) hip_check(hipMemcpyAsync(B.d_zin.p, file.p + z_lo, (size_t)(z_hi - z_lo), hipMemcpyHostToDevice, c->stream), "H2D");
      hip_check(hipEventRecord(B.ev[1], c->stream), "event");
      if (!dev_blks.empty()) {
        hip_check(hipMemsetAsync(B.d_stat.p, 0xff, dev_blks.size() * 4, c->stream), "memset");
        hip_check(mkp_launch_inflate_auto(c->stream, B.d_zin.as<uint8_t>(), B.d_blk.as<MkpBgzfBlock>(), (uint32_t)dev_blks.size(), text,
            B.d_stat.as<uint32_t>()), "inflate launch");
        hip_check(mkp_launch_crc32(c->stream, B.d_zin.as<uint8_t>(), B.d_blk.as<MkpBgzfBlock>(), (uint32_t)dev_blks.size(), text,
            B.d_stat.as<uint32_t>()), "crc32 launch");
      }
    }
    hip_check(hipEventRecord(B.ev[2], c->stream), "event");
    if (!n) break;   // (nothing but empty blocks)
    B.pieces++;
    const uint32_t n_chunks = (n + MKP_BEDIN_CHUNK - 1) / MKP_BEDIN_CHUNK;
    B.d_cnt.ensure((size_t)n_chunks * 12);
    hip_check(hipMemsetAsync(words, 0, MKP_BEDIN_WORDS * 4, c->stream), "memset");
    hip_check(hipMemsetAsync(words + MKP_BEDIN_W_ERR_OFF, 0xff, 8, c->stream), "memset");
    hip_check(mkp_launch_bedmethyl_lines(c->stream, text, n, final_piece ? 1u : 0u, B.d_cnt.as<uint32_t>(), words), "bedMethyl line count launch");
    hip_check(hipEventRecord(B.ev[3], c->stream), "event");
    uint32_t w[MKP_BEDIN_WORDS];
    d2h_copy(w, words, sizeof(w), c->stream);
    if (!dev_blks.empty()) {
      std::vector<uint32_t> st(dev_blks.size());
      d2h_copy(st.data(), B.d_stat.p, st.size() * 4, c->stream);
      for (size_t k = 0; k < st.size(); k++) if (st[k]) throw Error(MKP_E_IO, "corrupt BGZF data: block " + std::to_string(blk_index[k]) + " of " + path
          + (st[k] == 0x100u ? " (CRC-32 mismatch)" : " (decoder status " + std::to_string(st[k]) + ")"));
    }
    const uint32_t n_lines = w[MKP_BEDIN_W_LINES], n_rows = w[MKP_BEDIN_W_ROWS], limit = w[MKP_BEDIN_W_LIMIT];
    if (n_rows > n_lines || n_lines > n || limit > n) throw Error(MKP_E_DEVICE, "device bedMethyl reader: inconsistent line counts for " + path);
    const size_t stride = ((size_t)std::max(n_rows, 1u) + 63) & ~(size_t)63;
    B.d_lines.ensure(((size_t)n_lines + 1) * 4); B.d_rows.ensure(stride * 44); B.d_runs.ensure(std::max<size_t>(n_rows, 1) * sizeof(MkpBedRun));
    B.d_names.ensure(n);
    const MkpRowsDev rows = rows_at(B.d_rows.as<uint32_t>(), stride);
    hip_check(mkp_launch_bedmethyl_parse(c->stream, text, n, n_lines, n_rows, limit, (uint32_t)std::min<uint64_t>(max_line, 0xffffffffu),
        B.d_cnt.as<uint32_t>(), B.d_lines.as<uint32_t>(), &rows, B.d_runs.as<MkpBedRun>(), B.d_names.as<uint8_t>(), words), "bedMethyl parse launch");
    hip_check(hipEventRecord(B.ev[4], c->stream), "event");
    d2h_copy(w, words, sizeof(w), c->stream);
    B.ms[1] += bedin_elapsed(B.ev[0], B.ev[1]); B.ms[2] += bedin_elapsed(B.ev[1], B.ev[2]);
    B.ms[3] += bedin_elapsed(B.ev[2], B.ev[3]) + bedin_elapsed(B.ev[3], B.ev[4]);
    // the runs of the piece, in file order
    const uint32_t n_runs = w[MKP_BEDIN_W_RUNS], name_bytes = w[MKP_BEDIN_W_NAME_BYTES];
    if (n_runs > n_rows || name_bytes > n) throw Error(MKP_E_DEVICE, "device bedMethyl reader: inconsistent run counts for " + path);
    std::vector<MkpBedRun> runs(n_runs); std::vector<uint8_t> names(name_bytes);
    d2h_copy(runs.data(), B.d_runs.p, runs.size() * sizeof(MkpBedRun), c->stream);
    d2h_copy(names.data(), B.d_names.p, names.size(), c->stream);
    std::sort(runs.begin(), runs.end(), [](const MkpBedRun& a, const MkpBedRun& b) { return a.row < b.row; });
    for (const MkpBedRun& r : runs) if ((uint64_t)r.name_off + r.name_len > name_bytes || r.row >= n_rows) throw Error(MKP_E_DEVICE,
        "device bedMethyl reader: a run outside its piece for " + path);
    uint32_t bits = w[MKP_BEDIN_W_ERR];
    std::string first_chrom; if (n_runs) first_chrom.assign((const char*)names.data() + runs[0].name_off, runs[0].name_len);
    const bool goes_on = n_runs && have_last && first_chrom == last_chrom;
    if (goes_on && w[MKP_BEDIN_W_FIRST_POS] < last_pos) bits |= MKP_BEDIN_ERR_ORDER;
    if (bits) { uint64_t off; memcpy(&off, w + MKP_BEDIN_W_ERR_OFF, 8);
      bedin_fail(c, text, limit, line_base, path, bits, off, max_line, have_last ? &last_chrom : nullptr, last_pos); }
    for (uint32_t k = 0; k < n_runs; k++) {
      const uint32_t first = runs[k].row, cnt = (k + 1 < n_runs ? runs[k + 1].row : n_rows) - first;
      const std::string chrom((const char*)names.data() + runs[k].name_off, runs[k].name_len);
      const uint32_t* p = B.d_rows.as<uint32_t>() + first;
      const RowCols r = {p, p + stride, p + 2 * stride, p + 3 * stride, p + 4 * stride, cnt,
          {p + 5 * stride, p + 6 * stride, p + 7 * stride, p + 8 * stride, p + 9 * stride, p + 10 * stride}};
      sink(chrom, r, k == 0 && goes_on);
      if (k + 1 == n_runs) { last_chrom = chrom; last_pos = w[MKP_BEDIN_W_LAST_POS]; have_last = true; }
    }
    // the unfinished tail to the front of the other buffer
    carry = final_piece ? 0u : n - limit;
    line_base += w[MKP_BEDIN_W_NL];
    if (carry) {
      B.d_text[cur ^ 1].ensure(text_cap);
      hip_check(hipMemcpyAsync(B.d_text[cur ^ 1].p, text + limit, carry, hipMemcpyDeviceToDevice, c->stream), "D2D");
      cur ^= 1;
    }
  }
  hip_check(hipStreamSynchronize(c->stream), "sync");
}

}  // namespace

extern "C" {

int mkp_internal_bedmethyl_in_stats(mkp_ctx* c, int reset, double ms_out[4], uint64_t* pieces) {
  if (!c) return MKP_E_INVALID;
  if (ms_out) for (int k = 0; k < 4; k++) ms_out[k] = c->bedin.ms[k];
  if (pieces) *pieces = c->bedin.pieces;
  if (reset) { for (double& v : c->bedin.ms) v = 0; c->bedin.pieces = 0; }
  return MKP_OK;
}

int mkp_merge_add_file(mkp_ctx* c, const char* path, const char* const* contig_names, uint32_t n_names, uint64_t* n_rows) {
  if (!c || !path || (!contig_names && n_names)) return MKP_E_INVALID;
  if (n_rows) *n_rows = 0;
  return guarded(c, [&]() {
    mkp_ctx::Merge& M = c->merge;
    rt_need_open(M, kMergeWords);
    std::map<std::string, int32_t> tid_of;   // (the first of two equal names, as the sizes table of the command)
    for (uint32_t k = 0; k < n_names; k++) { if (!contig_names[k]) throw Error(MKP_E_INVALID, "contig name " + std::to_string(k) + " is NULL");
      tid_of.emplace(contig_names[k], (int32_t)k); }
    uint64_t total = 0;
    bedin_read_file(c, path, [&](const std::string& chrom, const RowCols& r, bool) {
      auto it = tid_of.find(chrom); const int32_t tid = it == tid_of.end() ? -1 : it->second;
      const uint64_t len = merge_contig_len(M, tid);
      uint64_t n_kept = 0;
      if (len && r.n) {   // the rows in front of the contig's length
        uint32_t* misc = M.d_misc.as<uint32_t>();
        hip_check(mkp_launch_merge_rows_below(c->stream, r.pos, (uint32_t)r.n, (uint32_t)len, misc + 2), "bedmethyl merge launch");
        uint32_t below = 0; d2h_copy(&below, misc + 2, 4, c->stream); n_kept = below;
      }
      merge_add(c, tid, r, n_kept);
      total += r.n;
    });
    if (n_rows) *n_rows = total;
  });
}

int mkp_bedmethyl_read_device(mkp_ctx* c, const char* path, mkp_bedmethyl_file** out) {
  if (!c || !path || !out) return MKP_E_INVALID;
  *out = nullptr;
  return guarded(c, [&]() {
    std::unique_ptr<mkp_bedmethyl_file> f(new mkp_bedmethyl_file());
    std::vector<uint32_t> tmp;
    bedin_read_file(c, path, [&](const std::string& chrom, const RowCols& r, bool goes_on) {
      if (goes_on && !f->runs.empty()) f->runs.back().n += r.n;
      else { mkp_bedmethyl_file::Run u; u.chrom = chrom; u.first = f->n_rows(); u.n = r.n; f->runs.push_back(u); }
      const size_t n = (size_t)r.n; tmp.resize(n);
      // file columns: pos, code_repr, n_valid, n_mod, then the six other counts
      const uint32_t* src[10] = {r.pos, r.code, r.n_valid, r.n_mod, r.rest[0], r.rest[1], r.rest[2], r.rest[3], r.rest[4], r.rest[5]};
      for (int k = 0; k < 10; k++) { d2h_copy(tmp.data(), src[k], n * 4, c->stream); f->col[k].insert(f->col[k].end(), tmp.begin(), tmp.end()); }
      d2h_copy(tmp.data(), r.info, n * 4, c->stream);
      for (size_t i = 0; i < n; i++) f->strand.push_back((uint8_t)"+-."[tmp[i] < 3u ? tmp[i] : 2u]);
      f->motif.insert(f->motif.end(), n, -1);
    });
    *out = f.release();
  });
}

}  // extern "C"

// ---- dmr pair (`modkit dmr pair` over regions, include/mkpileup.h): the table of sums stays in HBM between mkp_dmr_begin and mkp_dmr_get
namespace {

void dmr_need_sample(int sample) { if (sample != 0 && sample != 1) throw Error(MKP_E_INVALID, "sample must be 0 (a) or 1 (b)"); }

// the kernels over rows of contig `tid` that begin and end at position boundaries
void dmr_launch(mkp_ctx* c, int sample, int32_t tid, const RowCols& r) {
  mkp_ctx::Dmr& D = c->dmr;
  auto ref = D.ref.find(tid);
  if (ref == D.ref.end()) return;   // (no reference for the contig: its regions are not written)
  rt_launch(c, D, kDmrWords, tid, r.n, [&](uint32_t first, uint32_t n, hipEvent_t* ev) {
    uint32_t* misc = D.d_misc.as<uint32_t>();
    return mkp_launch_dmr(c->stream, r.pos, r.info, r.code, r.n_valid, r.n_mod, r.rest[0], (uint32_t)r.n, D.d_regions.as<MkpStatsRegion>() + first, n,
        D.d_lo.as<uint32_t>(), D.d_hi.as<uint32_t>(), D.d_cnt.as<uint32_t>(), D.d_off.as<unsigned long long>(),
        reinterpret_cast<unsigned long long*>(misc + MKP_STATS_MAX_CODES + 2), ref->second.buf.as<uint8_t>(), ref->second.off, ref->second.len, &D.prm,
        D.d_out.as<unsigned long long>() + (size_t)sample * D.n_regions * MKP_DMR_CELLS, D.d_seen.as<uint32_t>() + (size_t)sample * D.n_regions, misc,
        misc + MKP_STATS_MAX_CODES, ev);
  });
}

RowCols dmr_carry_rows(const mkp_ctx::Dmr::Carry& K) {
  const uint32_t* p = K.buf.as<uint32_t>(); const size_t s = mkp_ctx::Dmr::kCarryCap;
  return {p, p + s, p + 2 * s, p + 3 * s, p + 4 * s, K.n, {p + 5 * s, nullptr, nullptr, nullptr, nullptr, nullptr}};
}

// the rows held back of the sample's last piece: their position is whole now
void dmr_flush(mkp_ctx* c, int sample) {
  mkp_ctx::Dmr::Carry& K = c->dmr.carry[sample];
  if (K.n) dmr_launch(c, sample, K.tid, dmr_carry_rows(K));
  K.n = 0; K.tid = -1;
}

// rows [from, from + n) of r behind the carry's rows
void dmr_carry_append(mkp_ctx* c, mkp_ctx::Dmr::Carry& K, const RowCols& r, uint64_t from, uint32_t n) {
  if (K.n + n > mkp_ctx::Dmr::kCarryCap) throw Error(MKP_E_UNSUPPORTED, "dmr pair: more than " + std::to_string(mkp_ctx::Dmr::kCarryCap)
      + " rows at position " + std::to_string(K.pos) + " across a seam");
  K.buf.ensure((size_t)mkp_ctx::Dmr::kCarryCap * 6 * 4);
  uint32_t* d = K.buf.as<uint32_t>();
  const uint32_t* src[6] = {r.pos, r.info, r.code, r.n_valid, r.n_mod, r.rest[0]};
  for (int k = 0; k < 6; k++) hip_check(hipMemcpyAsync(d + (size_t)k * mkp_ctx::Dmr::kCarryCap + K.n, src[k] + from, (size_t)n * 4, hipMemcpyDeviceToDevice,
      c->stream), "D2D");
  K.n += n;
}

// One piece of contig `tid` of a sample, its rows on the device.  A seam may cut a position: the rows of the piece's last position are held
// back, and the rows at the front that continue the position held back join it first.  The kernels only ever see whole positions.
void dmr_add_piece(mkp_ctx* c, int sample, int32_t tid, const RowCols& r) {
  mkp_ctx::Dmr& D = c->dmr; mkp_ctx::Dmr::Carry& K = D.carry[sample];
  if (r.n > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 rows in one piece");
  if (!r.n) return;
  D.sample_tids[sample].insert(tid);
  constexpr uint32_t kEdge = 64;   // a position holds at most this many rows
  const uint32_t ne = (uint32_t)std::min<uint64_t>(r.n, kEdge);
  uint32_t front[kEdge], back[kEdge];
  d2h_copy(front, r.pos, (size_t)ne * 4, c->stream); d2h_copy(back, r.pos + (r.n - ne), (size_t)ne * 4, c->stream);
  auto too_many = [&](uint32_t pos) { return Error(MKP_E_UNSUPPORTED, "dmr pair: more than " + std::to_string(kEdge) + " rows at position "
      + std::to_string(pos) + " at the edge of a piece"); };
  uint64_t head = 0;
  if (K.n && K.tid == tid) {
    if (front[0] < K.pos) throw Error(MKP_E_INVALID, "dmr pair: the pieces of a contig must come in ascending order (" + std::to_string(front[0])
        + " follows " + std::to_string(K.pos) + ")");
    while (head < ne && front[head] == K.pos) head++;
    if (head == kEdge && r.n > kEdge) throw too_many(K.pos);
    if (head) dmr_carry_append(c, K, r, 0, (uint32_t)head);
    if (head == r.n) return;
  }
  dmr_flush(c, sample);
  const uint32_t last = back[ne - 1];
  uint64_t tail = 1;
  while (tail < ne && tail < r.n - head && back[ne - 1 - tail] == last) tail++;
  if (tail == kEdge && r.n - head > kEdge) throw too_many(last);
  K.tid = tid; K.pos = last;
  dmr_carry_append(c, K, r, r.n - tail, (uint32_t)tail);
  const uint64_t n = r.n - head - tail;
  if (n) dmr_launch(c, sample, tid, {r.pos + head, r.info + head, r.code + head, r.n_valid + head, r.n_mod + head, n,
      {r.rest[0] + head, nullptr, nullptr, nullptr, nullptr, nullptr}});
}

}  // namespace

extern "C" {

int mkp_internal_dmr_timing(mkp_ctx* c, int on, double ms_out[2]) { return c ? rt_timing(c, c->dmr, on, ms_out) : MKP_E_INVALID; }

uint32_t mkp_dmr_default_lookup(uint32_t* codes, uint8_t* code_bases, uint32_t cap) {
  const std::vector<DmrLookupEntry>& t = dmr_default_lookup();
  for (uint32_t k = 0; k < t.size() && k < cap; k++) { if (codes) codes[k] = t[k].code; if (code_bases) code_bases[k] = t[k].base; }
  return (uint32_t)t.size();
}

int mkp_dmr_begin(mkp_ctx* c, const mkp_region* regions, uint32_t n, const char* bases, uint32_t n_bases, const uint32_t* codes,
    const uint8_t* code_bases, uint32_t n_lookup, uint64_t min_valid_coverage, int respect_mask) {
  if (!c || (!regions && n) || (!bases && n_bases) || ((!codes || !code_bases) && n_lookup)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Dmr& D = c->dmr;
    D.open = false;
    if (n > 0x7fffffffu) throw Error(MKP_E_UNSUPPORTED, "more than 2^31 - 1 regions");
    for (uint32_t i = 0; i < n; i++) {
      if (regions[i].start > regions[i].end) throw Error(MKP_E_INVALID, "region " + std::to_string(i) + ": start > end");
      if (regions[i].strand_rule < 1 || regions[i].strand_rule > 3) throw Error(MKP_E_INVALID, "region " + std::to_string(i)
          + ": strand_rule must be 1 ('+'), 2 ('-') or 3 (both)");
    }
    MkpDmrParams P; memset(&P, 0, sizeof(P));
    P.min_cov = min_valid_coverage; P.mask = respect_mask ? 1u : 0u;
    if (!n_bases) throw Error(MKP_E_INVALID, "need to specify at least 1 modified base");
    for (uint32_t k = 0; k < n_bases; k++) {
      const char* at = strchr("ACGT", bases[k]);
      if (!at || !bases[k]) throw Error(MKP_E_INVALID, "modified base needs to be A, C, G, or T.");
      const uint32_t b = (uint32_t)(at - "ACGT");
      P.pos_set |= 1u << b; P.neg_set |= 1u << (3u - b);
    }
    for (uint32_t k = 0; k < n_lookup; k++) {   // a later entry for a code replaces an earlier one
      if (!codes[k]) throw Error(MKP_E_INVALID, "0 is not a mod code");
      if (code_bases[k] > 3) throw Error(MKP_E_INVALID, "a code's base is an index into ACGT");
      uint32_t at = 0; while (at < P.n_lookup && P.code[at] != codes[k]) at++;
      if (at == MKP_DMR_MAX_LOOKUP) throw Error(MKP_E_UNSUPPORTED, "dmr pair holds at most " + std::to_string(MKP_DMR_MAX_LOOKUP)
          + " codes in its code -> base table");
      P.code[at] = codes[k]; P.base[at] = code_bases[k]; if (at == P.n_lookup) P.n_lookup++;
    }
    // Only a code of one of the --base letters can ever take part: a '+' row needs its base under it, listed '+', a '-' row its complement,
    // listed '-', and either way that is a base of the positive set.  The kernel searches the table per row: keep what can match.
    uint32_t kept = 0;
    for (uint32_t k = 0; k < P.n_lookup; k++) if ((P.pos_set >> P.base[k]) & 1u) { P.code[kept] = P.code[k]; P.base[kept] = P.base[k]; kept++; }
    for (uint32_t k = kept; k < P.n_lookup; k++) { P.code[k] = 0; P.base[k] = 0; }
    P.n_lookup = kept;
    D.prm = P; D.n_regions = n; D.region_tid.resize(n);
    // the regions grouped by contig, caller order inside a contig; `out` = the caller's index
    std::vector<uint32_t> order(n); for (uint32_t i = 0; i < n; i++) { order[i] = i; D.region_tid[i] = regions[i].tid; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return regions[a].tid < regions[b].tid; });
    std::vector<MkpStatsRegion> dev(n); std::vector<int32_t> dev_tid(n);
    for (uint32_t k = 0; k < n; k++) { const mkp_region& g = regions[order[k]]; dev[k] = {g.start, g.end, g.strand_rule, order[k]}; dev_tid[k] = g.tid; }
    rt_group_by_tid(D, dev_tid);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(c->stream), "sync");   // (a previous session's kernels)
    for (auto& kv : D.ref) kv.second.buf.release();
    D.ref.clear();
    for (int s = 0; s < 2; s++) { D.carry[s].n = 0; D.carry[s].tid = -1; D.sample_tids[s].clear(); }
    const size_t n1 = std::max<size_t>(n, 1), m1 = std::max<size_t>(D.most_per_tid, 1);
    D.d_regions.ensure(n1 * sizeof(MkpStatsRegion)); D.d_out.ensure(2 * n1 * MKP_DMR_CELLS * 8); D.d_seen.ensure(2 * n1 * 4);
    D.d_misc.ensure(kStatsMiscBytes); D.d_lo.ensure(m1 * 4); D.d_hi.ensure(m1 * 4); D.d_cnt.ensure(m1 * 4); D.d_off.ensure((m1 + 1) * 8);
    h2d_copy(D.d_regions.p, dev.data(), (size_t)n * sizeof(MkpStatsRegion));
    hip_check(hipMemsetAsync(D.d_misc.p, 0, kStatsMiscBytes, c->stream), "memset");
    hip_check(hipMemsetAsync(D.d_out.p, 0, 2 * n1 * MKP_DMR_CELLS * 8, c->stream), "memset");
    hip_check(hipMemsetAsync(D.d_seen.p, 0, 2 * n1 * 4, c->stream), "memset");
    hip_check(hipStreamSynchronize(c->stream), "sync");
    D.open = true;
  });
}

int mkp_dmr_set_reference(mkp_ctx* c, int32_t tid, const uint8_t* bytes, uint32_t offset, uint32_t len) {
  if (!c || (!bytes && len)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Dmr& D = c->dmr;
    rt_need_open(D, kDmrWords);
    if (tid < 0) throw Error(MKP_E_INVALID, "the reference of a contig needs its tid");
    if ((uint64_t)offset + len > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "reference span beyond 2^32 - 1");
    if (D.sample_tids[0].count(tid) || D.sample_tids[1].count(tid)) throw Error(MKP_E_INVALID, "mkp_dmr_set_reference comes before the contig's rows");
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    mkp_ctx::Dmr::Ref& R = D.ref[tid];
    R.buf.ensure(std::max<size_t>(len, 1)); R.off = offset; R.len = len;
    h2d_copy(R.buf.p, bytes, len);
  });
}

int mkp_dmr_add_rows(mkp_ctx* c, int sample, int32_t tid, const mkp_rows* rows) {
  if (!c || !rows) return MKP_E_INVALID;
  return guarded(c, [&]() { dmr_need_sample(sample); dmr_add_piece(c, sample, tid, rt_upload_rows(c, c->dmr, kDmrWords, rows, 6)); });
}

int mkp_dmr_add_resident(mkp_ctx* c, int sample) {
  if (!c) return MKP_E_INVALID;
  return guarded(c, [&]() { dmr_need_sample(sample); dmr_add_piece(c, sample, c->shard.tid, rt_resident_rows(c, c->dmr, kDmrWords)); });
}

int mkp_dmr_add_file(mkp_ctx* c, int sample, const char* path, const char* const* contig_names, uint32_t n_names, uint64_t* n_rows) {
  if (!c || !path || (!contig_names && n_names)) return MKP_E_INVALID;
  if (n_rows) *n_rows = 0;
  return guarded(c, [&]() {
    dmr_need_sample(sample);
    rt_need_open(c->dmr, kDmrWords);
    std::map<std::string, int32_t> tid_of;   // (the first of two equal names)
    for (uint32_t k = 0; k < n_names; k++) { if (!contig_names[k]) throw Error(MKP_E_INVALID, "contig name " + std::to_string(k) + " is NULL");
      tid_of.emplace(contig_names[k], (int32_t)k); }
    uint64_t total = 0;
    bedin_read_file(c, path, [&](const std::string& chrom, const RowCols& r, bool) {
      auto it = tid_of.find(chrom);
      total += r.n;
      if (it != tid_of.end()) dmr_add_piece(c, sample, it->second, r);
    });
    dmr_flush(c, sample);   // (the reader's buffers are the next file's)
    if (n_rows) *n_rows = total;
  });
}

int mkp_dmr_get(mkp_ctx* c, mkp_dmr_out* out) {
  if (!c || !out) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::Dmr& D = c->dmr;
    rt_need_open(D, kDmrWords);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    for (int s = 0; s < 2; s++) dmr_flush(c, s);
    uint32_t misc[kStatsMiscBytes / 4];
    d2h_copy(misc, D.d_misc.p, sizeof(misc), c->stream);
    rt_check_codes(misc, kDmrWords);
    const uint32_t n = D.n_regions;
    std::vector<uint64_t> tab((size_t)2 * n * MKP_DMR_CELLS); std::vector<uint32_t> seen((size_t)2 * n);
    d2h_copy(tab.data(), D.d_out.p, tab.size() * 8, c->stream); d2h_copy(seen.data(), D.d_seen.p, seen.size() * 4, c->stream);
    uint32_t any = 0; for (uint32_t m : seen) any |= m & ~MKP_DMR_SEEN_BAD;
    const std::vector<std::pair<uint32_t, uint32_t>> cols = rt_columns(misc, any);   // code, slot
    const size_t nc = cols.size();
    D.h_codes.resize(nc); for (size_t k = 0; k < nc; k++) D.h_codes[k] = cols[k].first;
    D.h_ref.resize(n); D.h_state.resize(n); D.h_score.resize(n);
    for (uint32_t r = 0; r < n; r++) D.h_ref[r] = D.region_tid[r] >= 0 && D.ref.count(D.region_tid[r]) ? 1 : 0;
    for (int s = 0; s < 2; s++) {
      D.h_mod[s].assign((size_t)n * nc, 0); D.h_has_code[s].assign((size_t)n * nc, 0); D.h_total[s].resize(n); D.h_rows[s].resize(n);
      D.h_bad[s].resize(n); D.h_contig[s].resize(n);
      for (uint32_t r = 0; r < n; r++) {
        const uint64_t* line = &tab[((size_t)s * n + r) * MKP_DMR_CELLS]; const uint32_t m = seen[(size_t)s * n + r];
        for (size_t k = 0; k < nc; k++) { D.h_mod[s][(size_t)r * nc + k] = line[cols[k].second]; D.h_has_code[s][(size_t)r * nc + k] = (m >> cols[k].second) & 1u; }
        D.h_total[s][r] = line[MKP_DMR_CELL_TOTAL]; D.h_rows[s][r] = line[MKP_DMR_CELL_ROWS]; D.h_bad[s][r] = (m & MKP_DMR_SEEN_BAD) ? 1 : 0;
        D.h_contig[s][r] = D.region_tid[r] >= 0 && D.sample_tids[s].count(D.region_tid[r]) ? 1 : 0;
      }
    }
    out->n_regions = n; out->n_codes = (uint32_t)nc; out->code_repr = D.h_codes.data();
    for (int s = 0; s < 2; s++) { out->n_mod[s] = D.h_mod[s].data(); out->has_code[s] = D.h_has_code[s].data(); out->total[s] = D.h_total[s].data();
      out->n_rows[s] = D.h_rows[s].data(); out->bad[s] = D.h_bad[s].data(); out->contig_has_rows[s] = D.h_contig[s].data(); }
    out->has_reference = D.h_ref.data();
    dmr_judge(*out, D.h_score.data(), D.h_state.data());
    out->score = D.h_score.data(); out->state = D.h_state.data();
  });
}

}  // extern "C"

// ---- dmr sites (`modkit dmr pair` without -r, include/mkpileup.h): both tables' row columns stay in HBM per contig between
// mkp_dmr_sites_begin and mkp_dmr_sites_get, which runs the stages of mkp_dmr_sites.hip
namespace {

// device buffers of one mkp_dmr_sites_get, released when it returns or throws
struct ScopedBufs {
  std::vector<std::unique_ptr<DevBuf>> all;
  template <class T> T* get(size_t n) { all.emplace_back(new DevBuf()); all.back()->ensure(std::max<size_t>(n, 1) * sizeof(T)); return all.back()->as<T>(); }
  ~ScopedBufs() { for (auto& b : all) b->release(); }
};

// rows on the device behind the rows R of one (sample, contig); a contig's pieces come in ascending order.  what: the command; *row_bytes: the
// bytes of all the session's row columns, held to 3/4 of the device's memory
void dsites_rows_append(mkp_ctx* c, const char* what, mkp_ctx::DmrSites::Rows& R, uint64_t* row_bytes, const RowCols& r) {
  if (!r.n) return;
  if ((uint64_t)R.n + r.n > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 rows on one contig");
  uint32_t first = 0, last = 0;
  d2h_copy(&first, r.pos, 4, c->stream); d2h_copy(&last, r.pos + (r.n - 1), 4, c->stream);
  if (R.n && first < R.last_pos) throw Error(MKP_E_INVALID, std::string(what) + ": the pieces of a contig must come in ascending order ("
      + std::to_string(first) + " follows " + std::to_string(R.last_pos) + ")");
  const uint32_t* src[6] = {r.pos, r.info, r.code, r.n_valid, r.n_mod, r.rest[0]};
  const uint64_t need = (uint64_t)R.n + r.n;
  if (need > R.cap) {
    const uint64_t cap = ((std::max<uint64_t>(need, R.cap + R.cap / 2) + 63) & ~63ull);
    size_t free_b = 0, total_b = 0; hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    if (*row_bytes + (cap - R.cap) * 24 > (uint64_t)total_b / 4 * 3) throw Error(MKP_E_UNSUPPORTED, std::string(what) + ": the tables need more than "
        + std::to_string(total_b / 4 * 3 >> 20) + " MiB of device memory (24 bytes a row, all resident)");
    DevBuf grown; grown.ensure((size_t)cap * 24);
    for (int k = 0; k < 6 && R.n; k++) hip_check(hipMemcpyAsync(grown.as<uint32_t>() + (size_t)k * cap, R.col(k), (size_t)R.n * 4, hipMemcpyDeviceToDevice,
        c->stream), "D2D");
    hip_check(hipStreamSynchronize(c->stream), "sync");
    R.buf.release(); R.buf = grown; *row_bytes += (cap - R.cap) * 24; R.cap = cap;
  }
  for (int k = 0; k < 6; k++) hip_check(hipMemcpyAsync(R.buf.as<uint32_t>() + (size_t)k * R.cap + R.n, src[k], (size_t)r.n * 4, hipMemcpyDeviceToDevice,
      c->stream), "D2D");
  hip_check(hipStreamSynchronize(c->stream), "sync");   // (the source is the next call's upload buffer)
  R.n = (uint32_t)need; R.last_pos = last;
}

void dsites_append(mkp_ctx* c, int sample, int32_t tid, const RowCols& r) {
  mkp_ctx::DmrSites& D = c->dsites;
  if (tid < 0 || (size_t)tid >= D.names.size()) throw Error(MKP_E_INVALID, "dmr sites: rows of an unknown tid (" + std::to_string(tid) + ")");
  if (!r.n) return;
  dsites_rows_append(c, "dmr sites", D.contigs[tid].rows[sample], &D.row_bytes, r);
}

void dreps_append(mkp_ctx* c, uint32_t sample, int32_t tid, const RowCols& r) {
  mkp_ctx::DmrReps& D = c->dreps;
  if (tid < 0 || (size_t)tid >= D.names.size()) throw Error(MKP_E_INVALID, "dmr replicates: rows of an unknown tid (" + std::to_string(tid) + ")");
  if (!r.n) return;
  mkp_ctx::DmrReps::Contig& K = D.contigs[tid];
  K.rows.resize(D.n_side[0] + D.n_side[1]);
  dsites_rows_append(c, "dmr replicates", K.rows[sample], &D.row_bytes, r);
}

// a's sample `replicate` is sample `replicate` of the session, b's follows a's
uint32_t dreps_sample(const mkp_ctx::DmrReps& D, int side, int replicate) {
  if (side != 0 && side != 1) throw Error(MKP_E_INVALID, "side must be 0 (a) or 1 (b)");
  if (replicate < 0 || (uint32_t)replicate >= D.n_side[side]) throw Error(MKP_E_INVALID, "replicate " + std::to_string(replicate) + " of side "
      + (side ? "b" : "a") + ": the session holds " + std::to_string(D.n_side[side]));
  return (side ? D.n_side[0] : 0u) + (uint32_t)replicate;
}

// the checks of a mkp_dmr_sites_config and its row filter (mkp_dmr_sites_begin, mkp_dmr_reps_begin)
MkpDmrParams dsites_checked_params(const mkp_dmr_sites_config* cfg) {
  if (cfg->n_contigs > 0x7fffffffu) throw Error(MKP_E_UNSUPPORTED, "more than 2^31 - 1 contigs");
  MkpDmrParams P; memset(&P, 0, sizeof(P));
  P.min_cov = cfg->min_valid_coverage; P.mask = cfg->respect_mask ? 1u : 0u;
  if (!cfg->n_bases) throw Error(MKP_E_INVALID, "need to specify at least 1 modified base");
  for (uint32_t k = 0; k < cfg->n_bases; k++) {
    const char* at = strchr("ACGT", cfg->bases[k]);
    if (!at || !cfg->bases[k]) throw Error(MKP_E_INVALID, "modified base needs to be A, C, G, or T.");
    const uint32_t b = (uint32_t)(at - "ACGT");
    P.pos_set |= 1u << b; P.neg_set |= 1u << (3u - b);
  }
  for (uint32_t k = 0; k < cfg->n_lookup; k++) {   // a later entry for a code replaces an earlier one
    if (!cfg->codes[k]) throw Error(MKP_E_INVALID, "0 is not a mod code");
    if (cfg->code_bases[k] > 3) throw Error(MKP_E_INVALID, "a code's base is an index into ACGT");
    uint32_t at = 0; while (at < P.n_lookup && P.code[at] != cfg->codes[k]) at++;
    if (at == MKP_DMR_MAX_LOOKUP) throw Error(MKP_E_UNSUPPORTED, "dmr sites holds at most " + std::to_string(MKP_DMR_MAX_LOOKUP)
        + " codes in its code -> base table");
    P.code[at] = cfg->codes[k]; P.base[at] = cfg->code_bases[k]; if (at == P.n_lookup) P.n_lookup++;
  }
  // (only a code of one of the --base letters can ever take part: mkp_dmr_begin)
  uint32_t kept = 0;
  for (uint32_t k = 0; k < P.n_lookup; k++) if ((P.pos_set >> P.base[k]) & 1u) { P.code[kept] = P.code[k]; P.base[kept] = P.base[k]; kept++; }
  for (uint32_t k = kept; k < P.n_lookup; k++) { P.code[k] = 0; P.base[k] = 0; }
  P.n_lookup = kept;
  if (cfg->prior_alpha + cfg->prior_beta < 1.0) throw Error(MKP_E_INVALID, "alpha + beta must be > 1.0 for numerical stability");
  if (!(cfg->prior_alpha > 0.0) || !(cfg->prior_beta > 0.0) || std::isinf(cfg->prior_alpha) || std::isinf(cfg->prior_beta))
    throw Error(MKP_E_INVALID, "invalid beta parameters " + std::to_string(cfg->prior_alpha) + ", " + std::to_string(cfg->prior_beta));
  if (cfg->delta != cfg->delta) throw Error(MKP_E_INVALID, "--delta is not a number");
  if (!cfg->interval_size || cfg->interval_size > 0xffffffffull) throw Error(MKP_E_INVALID, "the interval size must be in [1, 2^32 - 1]");
  if (!cfg->batch_size) throw Error(MKP_E_INVALID, "the batch size must be at least 1");
  if (!cfg->have_max_coverages && !cfg->n_sample_records) throw Error(MKP_E_INVALID, "the number of sample records must be at least 1");
  return P;
}

double ms_between(std::chrono::steady_clock::time_point& t) {
  const auto now = std::chrono::steady_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(now - t).count();
  t = now;
  return ms;
}

}  // namespace

extern "C" {

int mkp_internal_dmr_sites_timing(mkp_ctx* c, double ms_out[7]) {
  if (!c || !ms_out) return MKP_E_INVALID;
  for (int k = 0; k < 7; k++) ms_out[k] = c->dsites.stage_ms[k];
  return MKP_OK;
}

// measurement aid: the sites of the last mkp_dmr_sites_get scored again by the same arithmetic on the host pool; *ms = the wall time, returns
// the number of sites whose three values differ in a bit from the device's (another libm: expected to be many, none an error)
int64_t mkp_internal_dmr_sites_host_ms(mkp_ctx* c, double* ms) {
  if (!c || !ms) return MKP_E_INVALID;
  mkp_ctx::DmrSites& D = c->dsites;
  const size_t n = D.h_pos.size(), nc = D.h_codes.size(), piece = 4096, np = (n + piece - 1) / piece;
  MkpDmrSiteMath M = D.math; M.max_cov[0] = D.used_max_cov[0]; M.max_cov[1] = D.used_max_cov[1];
  std::vector<uint64_t> differ(np, 0);
  auto t0 = std::chrono::steady_clock::now();
  HostPool::get().parallel(np, [&](size_t i) {
    for (size_t k = i * piece; k < std::min(n, (i + 1) * piece); k++) {
      uint64_t am[MKP_DMR_SITE_MAX_CODES] = {0}, bm[MKP_DMR_SITE_MAX_CODES] = {0}; double v[5];
      for (size_t j = 0; j < nc; j++) { am[j] = D.h_mod[0][k * nc + j]; bm[j] = D.h_mod[1][k * nc + j]; }
      dmr_site_score(am, D.h_has[0][k], D.h_total[0][k], bm, D.h_has[1][k], D.h_total[1][k], (uint32_t)nc, M, v);
      if (memcmp(&v[0], &D.h_score[k], 8) || memcmp(&v[3], &D.h_p[k], 8) || memcmp(&v[4], &D.h_effect[k], 8)) differ[i]++;
    }
  });
  *ms = ms_between(t0);
  uint64_t total = 0; for (uint64_t d : differ) total += d;
  return (int64_t)total;
}

int mkp_dmr_sites_begin(mkp_ctx* c, const mkp_dmr_sites_config* cfg) {
  if (!c || !cfg || (!cfg->contig_names && cfg->n_contigs) || (!cfg->bases && cfg->n_bases) || ((!cfg->codes || !cfg->code_bases) && cfg->n_lookup))
    return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::DmrSites& D = c->dsites;
    D.open = false;
    const MkpDmrParams P = dsites_checked_params(cfg);
    D.names.clear();
    for (uint32_t k = 0; k < cfg->n_contigs; k++) { if (!cfg->contig_names[k]) throw Error(MKP_E_INVALID, "contig name " + std::to_string(k) + " is NULL");
      D.names.push_back(cfg->contig_names[k]); }
    D.prm = P; D.have_max = cfg->have_max_coverages != 0; D.max_cov[0] = cfg->max_coverages[0]; D.max_cov[1] = cfg->max_coverages[1];
    D.math = dmr_site_math(cfg->prior_alpha, cfg->prior_beta, cfg->delta, D.max_cov);
    D.n_sample = cfg->n_sample_records; D.interval = cfg->interval_size; D.batch_size = cfg->batch_size;
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(c->stream), "sync");   // (a previous session's kernels)
    for (auto& kv : D.contigs) { kv.second.ref.release(); for (auto& r : kv.second.rows) r.buf.release(); }
    D.contigs.clear(); D.row_bytes = 0;
    D.d_misc.ensure(kStatsMiscBytes);
    D.open = true;
  });
}

int mkp_dmr_sites_set_reference(mkp_ctx* c, int32_t tid, const uint8_t* bytes, uint64_t len) {
  if (!c || (!bytes && len)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::DmrSites& D = c->dsites;
    rt_need_open(D, kDsitesWords);
    if (tid < 0 || (size_t)tid >= D.names.size()) throw Error(MKP_E_INVALID, "dmr sites: the reference of an unknown tid (" + std::to_string(tid) + ")");
    if (len > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "a contig beyond 2^32 - 1 bases");
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    mkp_ctx::DmrSites::Contig& K = D.contigs[tid];
    K.ref.ensure(std::max<size_t>((size_t)len, 1)); K.len = (uint32_t)len; K.has_ref = true;
    h2d_copy(K.ref.p, bytes, (size_t)len);
  });
}

int mkp_dmr_sites_add_rows(mkp_ctx* c, int sample, int32_t tid, const mkp_rows* rows) {
  if (!c || !rows) return MKP_E_INVALID;
  return guarded(c, [&]() { dmr_need_sample(sample); dsites_append(c, sample, tid, rt_upload_rows(c, c->dsites, kDsitesWords, rows, 6)); });
}

int mkp_dmr_sites_add_file(mkp_ctx* c, int sample, const char* path, uint64_t* n_rows) {
  if (!c || !path) return MKP_E_INVALID;
  if (n_rows) *n_rows = 0;
  return guarded(c, [&]() {
    dmr_need_sample(sample);
    mkp_ctx::DmrSites& D = c->dsites;
    rt_need_open(D, kDsitesWords);
    std::map<std::string, int32_t> tid_of;   // (the first of two equal names)
    for (size_t k = 0; k < D.names.size(); k++) tid_of.emplace(D.names[k], (int32_t)k);
    uint64_t total = 0;
    bedin_read_file(c, path, [&](const std::string& chrom, const RowCols& r, bool) {
      auto it = tid_of.find(chrom);
      total += r.n;
      if (it != tid_of.end()) dsites_append(c, sample, it->second, r);
    });
    if (n_rows) *n_rows = total;
  });
}

int mkp_dmr_sites_get(mkp_ctx* c, mkp_dmr_sites_out* out) {
  if (!c || !out) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::DmrSites& D = c->dsites;
    rt_need_open(D, kDsitesWords);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    hipStream_t st = c->stream;
    for (double& m : D.stage_ms) m = 0;
    auto clk = std::chrono::steady_clock::now();
    // the contigs of the walk: in the FASTA and in both tables, in byte order of their names
    std::vector<int32_t> tids;
    for (auto& kv : D.contigs) if (kv.second.has_ref && kv.second.rows[0].n && kv.second.rows[1].n) tids.push_back(kv.first);
    std::sort(tids.begin(), tids.end(), [&](int32_t a, int32_t b) { return D.names[a] != D.names[b] ? D.names[a] < D.names[b] : a < b; });
    if (tids.empty()) throw Error(MKP_E_INVALID, "need at least 1 contig");
    const size_t nt = tids.size();
    ScopedBufs bufs;

    // ---- listed counts, then the batch table
    std::vector<uint64_t> lens(nt), win_off(nt + 1, 0);
    for (size_t k = 0; k < nt; k++) { lens[k] = D.contigs[tids[k]].len; win_off[k + 1] = win_off[k] + dmr_sites_windows(lens[k], D.interval); }
    std::vector<uint32_t> counts((size_t)win_off[nt]);
    { uint32_t* d_counts = bufs.get<uint32_t>(counts.size());
      for (size_t k = 0; k < nt; k++) { const auto& K = D.contigs[tids[k]];
        hip_check(mkp_launch_dmr_sites_listed(st, K.ref.as<uint8_t>(), K.len, D.interval, (uint32_t)(win_off[k + 1] - win_off[k]), &D.prm,
            d_counts + win_off[k]), "dmr sites listed launch"); }
      d2h_copy(counts.data(), d_counts, counts.size() * 4, st); }
    std::vector<mkp_dmr_sites_batch> plan;
    const uint64_t n_batches = dmr_sites_plan(lens.data(), counts.data(), (uint32_t)nt, D.interval, &plan);
    if (n_batches > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 batches");
    std::vector<size_t> ent_off(nt + 1, 0);
    std::vector<MkpDmrSitesBatch> table(plan.size());
    for (size_t e = 0; e < plan.size(); e++) { table[e] = {(uint32_t)plan[e].start, (uint32_t)plan[e].batch}; ent_off[plan[e].contig + 1] = e + 1; }
    MkpDmrSitesBatch* d_table = bufs.get<MkpDmrSitesBatch>(table.size());
    h2d_copy(d_table, table.data(), table.size() * sizeof(MkpDmrSitesBatch));
    D.stage_ms[0] = ms_between(clk);

    // ---- heads: row flags and sites per (sample, contig); the slots' codes are the run's
    hip_check(hipMemsetAsync(D.d_misc.p, 0, kStatsMiscBytes, st), "memset");
    uint32_t* misc_d = D.d_misc.as<uint32_t>();
    struct Side { uint8_t* rowflag; uint32_t *tile, *totals, *s_pos, *s_first, *s_total, *s_info; uint32_t n_sites = 0, n_part = 0; };
    std::vector<Side> sides(2 * nt);
    for (size_t k = 0; k < nt; k++) for (int s = 0; s < 2; s++) {
      const auto& K = D.contigs[tids[k]]; const auto& R = K.rows[s]; Side& S = sides[2 * k + s];
      const size_t n = R.n, n_tiles = (n + MKP_DMRS_TILE - 1) / MKP_DMRS_TILE;
      S.rowflag = bufs.get<uint8_t>(n); S.tile = bufs.get<uint32_t>(2 * n_tiles); S.totals = bufs.get<uint32_t>(2);
      S.s_pos = bufs.get<uint32_t>(n); S.s_first = bufs.get<uint32_t>(n); S.s_total = bufs.get<uint32_t>(n); S.s_info = bufs.get<uint32_t>(n);
      hip_check(mkp_launch_dmr_sites_heads(st, R.col(0), R.col(1), R.col(2), R.col(3), R.col(4), R.col(5), R.n, K.ref.as<uint8_t>(), K.len, &D.prm,
          misc_d, misc_d + MKP_STATS_MAX_CODES, S.rowflag, S.tile, S.totals, S.s_pos, S.s_first, S.s_total, S.s_info), "dmr sites heads launch");
    }
    for (Side& S : sides) { uint32_t t[2]; d2h_copy(t, S.totals, 8, st); S.n_sites = t[0]; S.n_part = t[1]; }
    uint32_t misc[kStatsMiscBytes / 4];
    d2h_copy(misc, D.d_misc.p, sizeof(misc), st);
    rt_check_codes(misc, kDsitesWords);
    uint32_t any = 0; for (uint32_t s = 0; s < MKP_STATS_MAX_CODES; s++) if (misc[s]) any |= 1u << s;
    const std::vector<std::pair<uint32_t, uint32_t>> cols = rt_columns(misc, any);   // code, slot
    const uint32_t nc = (uint32_t)cols.size();
    unsigned long long col_of_slot = 0;
    D.h_codes.resize(nc);
    for (uint32_t k = 0; k < nc; k++) { D.h_codes[k] = cols[k].first; col_of_slot |= (unsigned long long)k << (4u * cols[k].second); }
    D.stage_ms[1] = ms_between(clk);

    // ---- the max coverages: given, or the 95th percentile of the coverages of the participating rows of the first super-batches
    uint32_t max_cov[2] = {D.max_cov[0], D.max_cov[1]}; uint64_t n_sampled[2] = {0, 0};
    if (!D.have_max) {
      const size_t ne = plan.size();
      std::vector<uint32_t> row_at[2], before[2];
      for (int s = 0; s < 2; s++) { row_at[s].resize(ne); before[s].resize(ne); }
      { uint32_t* d_at = bufs.get<uint32_t>(2 * ne); uint32_t* d_before = bufs.get<uint32_t>(2 * ne);
        for (size_t k = 0; k < nt; k++) for (int s = 0; s < 2; s++) { const auto& R = D.contigs[tids[k]].rows[s]; const Side& S = sides[2 * k + s];
          hip_check(mkp_launch_dmr_sites_bounds(st, R.col(0), S.rowflag, R.n, S.tile, S.totals, d_table + ent_off[k], (uint32_t)(ent_off[k + 1] - ent_off[k]),
              d_at + s * ne + ent_off[k], d_before + s * ne + ent_off[k]), "dmr sites bounds launch"); }
        for (int s = 0; s < 2; s++) { d2h_copy(row_at[s].data(), d_at + s * ne, ne * 4, st); d2h_copy(before[s].data(), d_before + s * ne, ne * 4, st); } }
      // the first super-batch behind which both samples hold n_sample values; the entries up to it are a prefix of the walk
      size_t stop = ne;   // entries [0, stop) are sampled
      { uint64_t have[2] = {0, 0}; size_t e = 0;
        while (e < ne) {
          const uint64_t sb = plan[e].batch / D.batch_size;
          for (; e < ne && plan[e].batch / D.batch_size == sb; e++) for (int s = 0; s < 2; s++) {
            const size_t k = plan[e].contig; const bool last_of_contig = e + 1 == ent_off[k + 1];
            have[s] += (last_of_contig ? sides[2 * k + s].n_part : before[s][e + 1]) - before[s][e];
          }
          if (std::min(have[0], have[1]) >= D.n_sample) { stop = e; break; }
        }
        n_sampled[0] = have[0]; n_sampled[1] = have[1]; }
      for (int s = 0; s < 2; s++) {
        if (n_sampled[s] < 2) throw Error(MKP_E_INVALID, "too few data points to calculate percentile, got " + std::to_string(n_sampled[s])
            + " (the max coverages are estimated from the participating rows of sample " + (s ? "b" : "a") + ": give --max-coverages)");
        if (n_sampled[s] > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 sampled coverages");
        uint32_t* d_cov = bufs.get<uint32_t>((size_t)n_sampled[s]); uint32_t* d_cursor = bufs.get<uint32_t>(1);
        hip_check(hipMemsetAsync(d_cursor, 0, 4, st), "memset");
        for (size_t k = 0; k < nt; k++) {
          const auto& R = D.contigs[tids[k]].rows[s];
          const uint32_t n_front = stop >= ent_off[k + 1] ? R.n : stop <= ent_off[k] ? 0u : row_at[s][stop];
          hip_check(mkp_launch_dmr_sites_coverages(st, sides[2 * k + s].rowflag, R.col(3), n_front, d_cursor, d_cov, (uint32_t)n_sampled[s]),
              "dmr sites coverages launch");
        }
        std::vector<uint32_t> cov((size_t)n_sampled[s]); uint32_t got = 0;
        d2h_copy(&got, d_cursor, 4, st); d2h_copy(cov.data(), d_cov, cov.size() * 4, st);
        if (got != n_sampled[s]) throw Error(MKP_E_DEVICE, "dmr sites: the coverage sample holds " + std::to_string(got) + " values, "
            + std::to_string(n_sampled[s]) + " were counted");
        std::vector<float> xs(cov.size()); for (size_t i = 0; i < cov.size(); i++) xs[i] = (float)cov[i];
        std::sort(xs.begin(), xs.end());
        float q = 0; if (mkp_percentile(xs.data(), xs.size(), 0.95f, &q) != MKP_OK) throw Error(MKP_E_INVALID, "percentile of the sampled coverages failed");
        max_cov[s] = (uint32_t)floorf(q);
      }
    }
    MkpDmrSiteMath math = D.math;
    for (int s = 0; s < 2; s++) { max_cov[s] = std::min<uint32_t>(max_cov[s], MKP_DMR_SITE_MAX_COV); math.max_cov[s] = max_cov[s]; }
    D.stage_ms[2] = ms_between(clk);

    // ---- bad batches of either sample, then per contig the join and the score
    uint32_t* d_bad = bufs.get<uint32_t>((size_t)n_batches);
    hip_check(hipMemsetAsync(d_bad, 0, std::max<size_t>((size_t)n_batches, 1) * 4, st), "memset");
    for (size_t k = 0; k < nt; k++) for (int s = 0; s < 2; s++) { const Side& S = sides[2 * k + s];
      hip_check(mkp_launch_dmr_sites_bad(st, S.s_pos, S.s_info, S.n_sites, d_table + ent_off[k], (uint32_t)(ent_off[k + 1] - ent_off[k]), d_bad),
          "dmr sites bad launch"); }
    std::vector<uint32_t> bad((size_t)n_batches);
    d2h_copy(bad.data(), d_bad, bad.size() * 4, st);
    uint64_t n_dropped = 0; for (uint32_t b : bad) if (b) n_dropped++;
    struct Joined { uint32_t *pair_a, *pair_b, n_pairs = 0; };
    std::vector<Joined> joined(nt); std::vector<MkpDmrSitesPairs> outs(nt);
    for (size_t k = 0; k < nt; k++) {
      const Side &A = sides[2 * k], &B = sides[2 * k + 1]; Joined& J = joined[k];
      const size_t n_tiles = ((size_t)A.n_sites + MKP_DMRS_TILE - 1) / MKP_DMRS_TILE;
      uint32_t* partner = bufs.get<uint32_t>(A.n_sites); uint32_t* tile = bufs.get<uint32_t>(2 * n_tiles); uint32_t* totals = bufs.get<uint32_t>(2);
      J.pair_a = bufs.get<uint32_t>(A.n_sites); J.pair_b = bufs.get<uint32_t>(A.n_sites);
      hip_check(mkp_launch_dmr_sites_join(st, A.s_pos, A.n_sites, B.s_pos, B.n_sites, d_table + ent_off[k], (uint32_t)(ent_off[k + 1] - ent_off[k]), d_bad,
          partner, tile, totals, J.pair_a, J.pair_b), "dmr sites join launch");
      uint32_t t[2]; d2h_copy(t, totals, 8, st); J.n_pairs = t[0];
      const size_t n = J.n_pairs; MkpDmrSitesPairs& O = outs[k];   // (the pairs' output, allocated outside the score stage's clock)
      O.pos = bufs.get<uint32_t>(n); O.info = bufs.get<uint32_t>(n); O.has = bufs.get<uint32_t>(n); O.total_a = bufs.get<uint32_t>(n);
      O.total_b = bufs.get<uint32_t>(n); O.cnt = bufs.get<uint32_t>(n * 2 * nc); O.score = bufs.get<double>(n); O.pvalue = bufs.get<double>(n);
      O.effect = bufs.get<double>(n);
    }
    D.stage_ms[3] = ms_between(clk);

    for (size_t k = 0; k < nt; k++) {
      const auto& K = D.contigs[tids[k]]; const Side &A = sides[2 * k], &B = sides[2 * k + 1]; const Joined& J = joined[k];
      const MkpDmrSitesPairs& O = outs[k];
      const MkpDmrSitesSample sa = {K.rows[0].col(0), K.rows[0].col(4), A.rowflag, K.rows[0].n, A.s_pos, A.s_first, A.s_total, A.s_info};
      const MkpDmrSitesSample sb = {K.rows[1].col(0), K.rows[1].col(4), B.rowflag, K.rows[1].n, B.s_pos, B.s_first, B.s_total, B.s_info};
      hip_check(mkp_launch_dmr_sites_score(st, &sa, &sb, J.pair_a, J.pair_b, J.n_pairs, col_of_slot, nc, &math, &O), "dmr sites score launch");
    }
    hip_check(hipStreamSynchronize(st), "dmr sites score sync");
    D.stage_ms[4] = ms_between(clk);

    // ---- read-back, and the written sites in walk order
    uint64_t n_all = 0; for (const Joined& J : joined) n_all += J.n_pairs;
    D.h_tid.clear(); D.h_pos.clear(); D.h_strand.clear(); D.h_score.clear(); D.h_p.clear(); D.h_effect.clear();
    for (int s = 0; s < 2; s++) { D.h_total[s].clear(); D.h_mod[s].clear(); D.h_has[s].clear(); }
    D.h_tid.reserve(n_all); D.h_pos.reserve(n_all); D.h_score.reserve(n_all);
    uint64_t n_failed = 0; double read_ms = 0;
    std::vector<uint32_t> pos, info, has, ta, tb, cnt; std::vector<double> score, pv, eff;
    for (size_t k = 0; k < nt; k++) {
      const size_t n = joined[k].n_pairs; const MkpDmrSitesPairs& O = outs[k];
      auto t_read = std::chrono::steady_clock::now();
      pos.resize(n); info.resize(n); has.resize(n); ta.resize(n); tb.resize(n); cnt.resize(n * 2 * nc); score.resize(n); pv.resize(n); eff.resize(n);
      d2h_copy(pos.data(), O.pos, n * 4, st); d2h_copy(info.data(), O.info, n * 4, st); d2h_copy(has.data(), O.has, n * 4, st);
      d2h_copy(ta.data(), O.total_a, n * 4, st); d2h_copy(tb.data(), O.total_b, n * 4, st); d2h_copy(cnt.data(), O.cnt, n * 2 * nc * 4, st);
      d2h_copy(score.data(), O.score, n * 8, st); d2h_copy(pv.data(), O.pvalue, n * 8, st); d2h_copy(eff.data(), O.effect, n * 8, st);
      read_ms += ms_between(t_read);
      for (size_t i = 0; i < n; i++) {
        if (info[i] & MKP_DMRS_PAIR_FAILED) { n_failed++; continue; }
        D.h_tid.push_back(tids[k]); D.h_pos.push_back(pos[i]); D.h_strand.push_back((info[i] & MKP_DMRS_SITE_MINUS) ? '-' : '+');
        D.h_total[0].push_back(ta[i]); D.h_total[1].push_back(tb[i]); D.h_has[0].push_back(has[i] & 0xffffu); D.h_has[1].push_back(has[i] >> 16);
        for (int s = 0; s < 2; s++) D.h_mod[s].insert(D.h_mod[s].end(), cnt.begin() + (i * 2 + s) * nc, cnt.begin() + (i * 2 + s + 1) * nc);
        D.h_score.push_back(score[i]); D.h_p.push_back(pv[i]); D.h_effect.push_back(eff[i]);
      }
    }
    D.stage_ms[5] = read_ms; D.stage_ms[6] = ms_between(clk) - read_ms;
    memset(out, 0, sizeof(*out));
    out->n_sites = D.h_pos.size(); out->n_codes = nc; out->code_repr = D.h_codes.data();
    out->tid = D.h_tid.data(); out->pos = D.h_pos.data(); out->strand = D.h_strand.data();
    for (int s = 0; s < 2; s++) { out->total[s] = D.h_total[s].data(); out->n_mod[s] = D.h_mod[s].data(); out->has_code[s] = D.h_has[s].data();
      out->max_coverages[s] = max_cov[s]; out->n_sampled[s] = n_sampled[s]; }
    out->score = D.h_score.data(); out->map_pvalue = D.h_p.data(); out->effect_size = D.h_effect.data();
    out->n_batches = n_batches; out->n_batches_dropped = n_dropped; out->n_model_failures = n_failed;
    D.used_max_cov[0] = max_cov[0]; D.used_max_cov[1] = max_cov[1];
  });
}

}  // extern "C"

// ---- dmr replicates (`modkit dmr pair` without -r over several -a / -b tables, include/mkpileup.h): every table's row columns stay in HBM per
// contig between mkp_dmr_reps_begin and mkp_dmr_reps_get, which runs dmr sites' stages per sample and the stages of mkp_dmr_reps.hip
static_assert(MKP_DMRR_MAX_SIDE == MKP_DMR_REPS_MAX_SIDE, "the device's sample limit is the public one");

extern "C" {

int mkp_internal_dmr_reps_timing(mkp_ctx* c, double ms_out[9]) {
  if (!c || !ms_out) return MKP_E_INVALID;
  for (int k = 0; k < 9; k++) ms_out[k] = c->dreps.stage_ms[k];
  return MKP_OK;
}

int mkp_dmr_reps_begin(mkp_ctx* c, const mkp_dmr_sites_config* cfg, uint32_t n_a, uint32_t n_b, int cap_coverages) {
  if (!c || !cfg || (!cfg->contig_names && cfg->n_contigs) || (!cfg->bases && cfg->n_bases) || ((!cfg->codes || !cfg->code_bases) && cfg->n_lookup))
    return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::DmrReps& D = c->dreps;
    D.open = false;
    if (!n_a || !n_b) throw Error(MKP_E_INVALID, "must be at least 1 sample for 'a' and 'b'");
    if (n_a > MKP_DMRR_MAX_SIDE || n_b > MKP_DMRR_MAX_SIDE) throw Error(MKP_E_UNSUPPORTED, "dmr replicates holds at most "
        + std::to_string(MKP_DMRR_MAX_SIDE) + " tables a side (" + std::to_string(n_a) + " -a, " + std::to_string(n_b) + " -b)");
    const MkpDmrParams P = dsites_checked_params(cfg);
    D.names.clear();
    for (uint32_t k = 0; k < cfg->n_contigs; k++) { if (!cfg->contig_names[k]) throw Error(MKP_E_INVALID, "contig name " + std::to_string(k) + " is NULL");
      D.names.push_back(cfg->contig_names[k]); }
    D.prm = P; D.have_max = cfg->have_max_coverages != 0; D.max_cov[0] = cfg->max_coverages[0]; D.max_cov[1] = cfg->max_coverages[1];
    D.math = dmr_site_math(cfg->prior_alpha, cfg->prior_beta, cfg->delta, D.max_cov);
    D.n_sample = cfg->n_sample_records; D.interval = cfg->interval_size; D.batch_size = cfg->batch_size;
    D.n_side[0] = n_a; D.n_side[1] = n_b; D.cap = cap_coverages != 0;
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    hip_check(hipStreamSynchronize(c->stream), "sync");   // (a previous session's kernels)
    for (auto& kv : D.contigs) { kv.second.ref.release(); for (auto& r : kv.second.rows) r.buf.release(); }
    D.contigs.clear(); D.row_bytes = 0;
    D.d_misc.ensure(kStatsMiscBytes);
    D.open = true;
  });
}

int mkp_dmr_reps_set_reference(mkp_ctx* c, int32_t tid, const uint8_t* bytes, uint64_t len) {
  if (!c || (!bytes && len)) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::DmrReps& D = c->dreps;
    rt_need_open(D, kDrepsWords);
    if (tid < 0 || (size_t)tid >= D.names.size()) throw Error(MKP_E_INVALID, "dmr replicates: the reference of an unknown tid (" + std::to_string(tid) + ")");
    if (len > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "a contig beyond 2^32 - 1 bases");
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    mkp_ctx::DmrReps::Contig& K = D.contigs[tid];
    K.ref.ensure(std::max<size_t>((size_t)len, 1)); K.len = (uint32_t)len; K.has_ref = true;
    h2d_copy(K.ref.p, bytes, (size_t)len);
  });
}

int mkp_dmr_reps_add_rows(mkp_ctx* c, int side, int replicate, int32_t tid, const mkp_rows* rows) {
  if (!c || !rows) return MKP_E_INVALID;
  return guarded(c, [&]() {
    rt_need_open(c->dreps, kDrepsWords);
    const uint32_t sample = dreps_sample(c->dreps, side, replicate);
    dreps_append(c, sample, tid, rt_upload_rows(c, c->dreps, kDrepsWords, rows, 6));
  });
}

int mkp_dmr_reps_add_file(mkp_ctx* c, int side, int replicate, const char* path, uint64_t* n_rows) {
  if (!c || !path) return MKP_E_INVALID;
  if (n_rows) *n_rows = 0;
  return guarded(c, [&]() {
    mkp_ctx::DmrReps& D = c->dreps;
    rt_need_open(D, kDrepsWords);
    const uint32_t sample = dreps_sample(D, side, replicate);
    std::map<std::string, int32_t> tid_of;   // (the first of two equal names)
    for (size_t k = 0; k < D.names.size(); k++) tid_of.emplace(D.names[k], (int32_t)k);
    uint64_t total = 0;
    bedin_read_file(c, path, [&](const std::string& chrom, const RowCols& r, bool) {
      auto it = tid_of.find(chrom);
      total += r.n;
      if (it != tid_of.end()) dreps_append(c, sample, it->second, r);
    });
    if (n_rows) *n_rows = total;
  });
}

int mkp_dmr_reps_get(mkp_ctx* c, mkp_dmr_reps_out* out) {
  if (!c || !out) return MKP_E_INVALID;
  return guarded(c, [&]() {
    mkp_ctx::DmrReps& D = c->dreps;
    rt_need_open(D, kDrepsWords);
    hip_check(hipSetDevice(c->device), "hipSetDevice");
    hipStream_t st = c->stream;
    for (double& m : D.stage_ms) m = 0;
    auto clk = std::chrono::steady_clock::now();
    const uint32_t n_a = D.n_side[0], n_b = D.n_side[1], ns = n_a + n_b;
    const bool matched = n_a == n_b && n_a > 1;
    const uint32_t rep_stride = matched ? n_a : 0u;
    auto side_of = [&](uint32_t s) { return s < n_a ? 0 : 1; };
    // the contigs of the walk: in the FASTA, in at least one table of a and in at least one of b, in byte order of their names
    std::vector<int32_t> tids;
    for (auto& kv : D.contigs) {
      bool has[2] = {false, false};
      kv.second.rows.resize(ns);
      for (uint32_t s = 0; s < ns; s++) if (kv.second.rows[s].n) has[side_of(s)] = true;
      if (kv.second.has_ref && has[0] && has[1]) tids.push_back(kv.first);
    }
    std::sort(tids.begin(), tids.end(), [&](int32_t a, int32_t b) { return D.names[a] != D.names[b] ? D.names[a] < D.names[b] : a < b; });
    if (tids.empty()) throw Error(MKP_E_INVALID, "need at least 1 contig");
    const size_t nt = tids.size();
    ScopedBufs bufs;

    // ---- listed counts, then the batch table (the walk depends on the reference alone)
    std::vector<uint64_t> lens(nt), win_off(nt + 1, 0);
    for (size_t k = 0; k < nt; k++) { lens[k] = D.contigs[tids[k]].len; win_off[k + 1] = win_off[k] + dmr_sites_windows(lens[k], D.interval); }
    std::vector<uint32_t> counts((size_t)win_off[nt]);
    { uint32_t* d_counts = bufs.get<uint32_t>(counts.size());
      for (size_t k = 0; k < nt; k++) { const auto& K = D.contigs[tids[k]];
        hip_check(mkp_launch_dmr_sites_listed(st, K.ref.as<uint8_t>(), K.len, D.interval, (uint32_t)(win_off[k + 1] - win_off[k]), &D.prm,
            d_counts + win_off[k]), "dmr replicates listed launch"); }
      d2h_copy(counts.data(), d_counts, counts.size() * 4, st); }
    std::vector<mkp_dmr_sites_batch> plan;
    const uint64_t n_batches = dmr_sites_plan(lens.data(), counts.data(), (uint32_t)nt, D.interval, &plan);
    if (n_batches > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 batches");
    std::vector<size_t> ent_off(nt + 1, 0);
    std::vector<MkpDmrSitesBatch> table(plan.size());
    for (size_t e = 0; e < plan.size(); e++) { table[e] = {(uint32_t)plan[e].start, (uint32_t)plan[e].batch}; ent_off[plan[e].contig + 1] = e + 1; }
    MkpDmrSitesBatch* d_table = bufs.get<MkpDmrSitesBatch>(table.size());
    h2d_copy(d_table, table.data(), table.size() * sizeof(MkpDmrSitesBatch));
    D.stage_ms[0] = ms_between(clk);

    // ---- heads: row flags and sites per (contig, sample); the slots' codes are the run's
    hip_check(hipMemsetAsync(D.d_misc.p, 0, kStatsMiscBytes, st), "memset");
    uint32_t* misc_d = D.d_misc.as<uint32_t>();
    struct Sample { uint8_t* rowflag; uint32_t *tile, *totals, *s_pos, *s_first, *s_total, *s_info; uint32_t n_sites = 0, n_part = 0; };
    std::vector<Sample> smp(ns * nt);   // [contig * ns + sample]
    for (size_t k = 0; k < nt; k++) for (uint32_t s = 0; s < ns; s++) {
      const auto& K = D.contigs[tids[k]]; const auto& R = K.rows[s]; Sample& S = smp[k * ns + s];
      const size_t n = R.n, n_tiles = (n + MKP_DMRS_TILE - 1) / MKP_DMRS_TILE;
      S.rowflag = bufs.get<uint8_t>(n); S.tile = bufs.get<uint32_t>(2 * n_tiles); S.totals = bufs.get<uint32_t>(2);
      S.s_pos = bufs.get<uint32_t>(n); S.s_first = bufs.get<uint32_t>(n); S.s_total = bufs.get<uint32_t>(n); S.s_info = bufs.get<uint32_t>(n);
      hip_check(mkp_launch_dmr_sites_heads(st, R.col(0), R.col(1), R.col(2), R.col(3), R.col(4), R.col(5), R.n, K.ref.as<uint8_t>(), K.len, &D.prm,
          misc_d, misc_d + MKP_STATS_MAX_CODES, S.rowflag, S.tile, S.totals, S.s_pos, S.s_first, S.s_total, S.s_info), "dmr replicates heads launch");
    }
    for (Sample& S : smp) { uint32_t t[2]; d2h_copy(t, S.totals, 8, st); S.n_sites = t[0]; S.n_part = t[1]; }
    uint32_t misc[kStatsMiscBytes / 4];
    d2h_copy(misc, D.d_misc.p, sizeof(misc), st);
    rt_check_codes(misc, kDrepsWords);
    uint32_t any = 0; for (uint32_t s = 0; s < MKP_STATS_MAX_CODES; s++) if (misc[s]) any |= 1u << s;
    const std::vector<std::pair<uint32_t, uint32_t>> cols = rt_columns(misc, any);   // code, slot
    const uint32_t nc = (uint32_t)cols.size();
    unsigned long long col_of_slot = 0;
    D.h_codes.resize(nc);
    for (uint32_t k = 0; k < nc; k++) { D.h_codes[k] = cols[k].first; col_of_slot |= (unsigned long long)k << (4u * cols[k].second); }
    D.stage_ms[1] = ms_between(clk);

    // ---- the max coverages: given, or the 95th percentile of the coverages of the participating rows of the first super-batches, pooled
    // over a side's samples
    uint32_t max_cov[2] = {D.max_cov[0], D.max_cov[1]}; uint64_t n_sampled[2] = {0, 0};
    if (!D.have_max) {
      const size_t ne = plan.size();
      std::vector<std::vector<uint32_t>> row_at(ns, std::vector<uint32_t>(ne)), before(ns, std::vector<uint32_t>(ne));
      { uint32_t* d_at = bufs.get<uint32_t>((size_t)ns * ne); uint32_t* d_before = bufs.get<uint32_t>((size_t)ns * ne);
        for (size_t k = 0; k < nt; k++) for (uint32_t s = 0; s < ns; s++) { const auto& R = D.contigs[tids[k]].rows[s]; const Sample& S = smp[k * ns + s];
          hip_check(mkp_launch_dmr_sites_bounds(st, R.col(0), S.rowflag, R.n, S.tile, S.totals, d_table + ent_off[k], (uint32_t)(ent_off[k + 1] - ent_off[k]),
              d_at + s * ne + ent_off[k], d_before + s * ne + ent_off[k]), "dmr replicates bounds launch"); }
        for (uint32_t s = 0; s < ns; s++) { d2h_copy(row_at[s].data(), d_at + s * ne, ne * 4, st); d2h_copy(before[s].data(), d_before + s * ne, ne * 4, st); } }
      // the first super-batch behind which both sides hold n_sample values; the entries up to it are a prefix of the walk
      size_t stop = ne;   // entries [0, stop) are sampled
      { uint64_t have[2] = {0, 0}; size_t e = 0;
        while (e < ne) {
          const uint64_t sb = plan[e].batch / D.batch_size;
          for (; e < ne && plan[e].batch / D.batch_size == sb; e++) for (uint32_t s = 0; s < ns; s++) {
            const size_t k = plan[e].contig; const bool last_of_contig = e + 1 == ent_off[k + 1];
            have[side_of(s)] += (last_of_contig ? smp[k * ns + s].n_part : before[s][e + 1]) - before[s][e];
          }
          if (std::min(have[0], have[1]) >= D.n_sample) { stop = e; break; }
        }
        n_sampled[0] = have[0]; n_sampled[1] = have[1]; }
      for (int side = 0; side < 2; side++) {
        if (n_sampled[side] < 2) throw Error(MKP_E_INVALID, "too few data points to calculate percentile, got " + std::to_string(n_sampled[side])
            + " (the max coverages are estimated from the participating rows of the " + (side ? "b" : "a") + " samples: give --max-coverages)");
        if (n_sampled[side] > 0xffffffffull) throw Error(MKP_E_UNSUPPORTED, "more than 2^32 - 1 sampled coverages");
        uint32_t* d_cov = bufs.get<uint32_t>((size_t)n_sampled[side]); uint32_t* d_cursor = bufs.get<uint32_t>(1);
        hip_check(hipMemsetAsync(d_cursor, 0, 4, st), "memset");
        for (size_t k = 0; k < nt; k++) for (uint32_t s = side ? n_a : 0u; s < (side ? ns : n_a); s++) {
          const auto& R = D.contigs[tids[k]].rows[s];
          const uint32_t n_front = stop >= ent_off[k + 1] ? R.n : stop <= ent_off[k] ? 0u : row_at[s][stop];
          hip_check(mkp_launch_dmr_sites_coverages(st, smp[k * ns + s].rowflag, R.col(3), n_front, d_cursor, d_cov, (uint32_t)n_sampled[side]),
              "dmr replicates coverages launch");
        }
        std::vector<uint32_t> cov((size_t)n_sampled[side]); uint32_t got = 0;
        d2h_copy(&got, d_cursor, 4, st); d2h_copy(cov.data(), d_cov, cov.size() * 4, st);
        if (got != n_sampled[side]) throw Error(MKP_E_DEVICE, "dmr replicates: the coverage sample holds " + std::to_string(got) + " values, "
            + std::to_string(n_sampled[side]) + " were counted");
        std::vector<float> xs(cov.size()); for (size_t i = 0; i < cov.size(); i++) xs[i] = (float)cov[i];
        std::sort(xs.begin(), xs.end());
        float q = 0; if (mkp_percentile(xs.data(), xs.size(), 0.95f, &q) != MKP_OK) throw Error(MKP_E_INVALID, "percentile of the sampled coverages failed");
        max_cov[side] = (uint32_t)floorf(q);
      }
    }
    // PMapEstimator::new: a side's max coverage times its number of tables unless --cap-coverages, then the cap of 300
    MkpDmrSiteMath math = D.math;
    for (int s = 0; s < 2; s++) {
      const uint64_t m = (uint64_t)max_cov[s] * (D.cap ? 1u : D.n_side[s]);
      max_cov[s] = (uint32_t)std::min<uint64_t>(m, MKP_DMR_SITE_MAX_COV); math.max_cov[s] = max_cov[s];
    }
    D.stage_ms[2] = ms_between(clk);

    // ---- bad batches of any sample, then per contig the two bitmaps, their join and the joined positions
    uint32_t* d_bad = bufs.get<uint32_t>((size_t)n_batches);
    hip_check(hipMemsetAsync(d_bad, 0, std::max<size_t>((size_t)n_batches, 1) * 4, st), "memset");
    for (size_t k = 0; k < nt; k++) for (uint32_t s = 0; s < ns; s++) { const Sample& S = smp[k * ns + s];
      hip_check(mkp_launch_dmr_sites_bad(st, S.s_pos, S.s_info, S.n_sites, d_table + ent_off[k], (uint32_t)(ent_off[k + 1] - ent_off[k]), d_bad),
          "dmr replicates bad launch"); }
    std::vector<uint32_t> bad((size_t)n_batches);
    d2h_copy(bad.data(), d_bad, bad.size() * 4, st);
    uint64_t n_dropped = 0; for (uint32_t b : bad) if (b) n_dropped++;
    uint64_t max_len = 0; for (uint64_t l : lens) max_len = std::max(max_len, l);
    const size_t max_words = (size_t)((max_len + 31) / 32), max_tiles = (max_words + MKP_DMRS_TILE - 1) / MKP_DMRS_TILE;
    uint32_t* d_bits[2] = {bufs.get<uint32_t>(max_words), bufs.get<uint32_t>(max_words)};   // (one pair, a contig after the other in stream order)
    uint32_t* d_word_tile = bufs.get<uint32_t>(2 * max_tiles); uint32_t* d_totals = bufs.get<uint32_t>(2);
    struct Joined { uint32_t* j_pos = nullptr; uint32_t n = 0; };
    std::vector<Joined> joined(nt);
    for (size_t k = 0; k < nt; k++) {
      Joined& J = joined[k];
      const uint32_t n_words = (uint32_t)((lens[k] + 31) / 32);
      for (int side = 0; side < 2; side++) hip_check(hipMemsetAsync(d_bits[side], 0, std::max<size_t>(n_words, 1) * 4, st), "memset");
      for (uint32_t s = 0; s < ns; s++) { const Sample& S = smp[k * ns + s];
        hip_check(mkp_launch_dmr_reps_mark(st, S.s_pos, S.n_sites, d_bits[side_of(s)], n_words), "dmr replicates mark launch"); }
      hip_check(mkp_launch_dmr_reps_join(st, d_bits[0], d_bits[1], n_words, d_table + ent_off[k], (uint32_t)(ent_off[k + 1] - ent_off[k]), d_bad, d_word_tile,
          d_totals), "dmr replicates join launch");
      uint32_t t[2]; d2h_copy(t, d_totals, 8, st); J.n = t[0];
      J.j_pos = bufs.get<uint32_t>(J.n);
      hip_check(mkp_launch_dmr_reps_list(st, d_bits[0], n_words, d_word_tile, J.j_pos, J.n), "dmr replicates list launch");
    }
    D.stage_ms[3] = ms_between(clk);

    // ---- gather: the collapsed and balanced counts and the replicates' counts of every joined site
    std::vector<MkpDmrRepsSites> outs(nt);
    MkpDmrRepsSample* d_samples = bufs.get<MkpDmrRepsSample>((size_t)nt * ns);
    { std::vector<MkpDmrRepsSample> h(nt * ns);
      for (size_t k = 0; k < nt; k++) for (uint32_t s = 0; s < ns; s++) { const auto& R = D.contigs[tids[k]].rows[s]; const Sample& S = smp[k * ns + s];
        h[k * ns + s] = {{R.col(0), R.col(4), S.rowflag, R.n, S.s_pos, S.s_first, S.s_total, S.s_info}, S.n_sites, 0u}; }
      h2d_copy(d_samples, h.data(), h.size() * sizeof(MkpDmrRepsSample)); }
    for (size_t k = 0; k < nt; k++) {
      const size_t n = joined[k].n; MkpDmrRepsSites& O = outs[k];
      O.pos = bufs.get<uint32_t>(n); O.info = bufs.get<uint32_t>(n); O.present = bufs.get<uint32_t>(n); O.pct = bufs.get<uint32_t>(n);
      O.has = bufs.get<uint32_t>(n); O.total = bufs.get<uint32_t>(2 * n); O.bal_total = bufs.get<uint32_t>(2 * n); O.cnt = bufs.get<uint32_t>(n * 2 * nc);
      O.bal_cnt = bufs.get<uint32_t>(n * 2 * nc); O.msum = bufs.get<uint32_t>(4 * n); O.rep = bufs.get<uint32_t>(n * 4 * rep_stride);
      O.n_rep = bufs.get<uint32_t>(n); O.score = bufs.get<double>(n); O.pvalue = bufs.get<double>(n); O.effect = bufs.get<double>(n);
      O.bal_pvalue = bufs.get<double>(n); O.bal_effect = bufs.get<double>(n); O.rep_pvalue = bufs.get<double>(n * rep_stride);
      O.rep_effect = bufs.get<double>(n * rep_stride);
      hip_check(mkp_launch_dmr_reps_gather(st, d_samples + k * ns, n_a, n_b, joined[k].j_pos, joined[k].n, col_of_slot, nc, rep_stride, &O),
          "dmr replicates gather launch");
    }
    hip_check(hipStreamSynchronize(st), "dmr replicates gather sync");
    D.stage_ms[4] = ms_between(clk);

    // ---- the task lists, then the p-values and the ratios
    struct Tasks { uint32_t* off = nullptr; uint32_t n[2] = {0, 0}; };
    std::vector<Tasks> tasks(nt);
    for (size_t k = 0; k < nt; k++) {
      const size_t n = joined[k].n, n_tiles = (n + MKP_DMRS_TILE - 1) / MKP_DMRS_TILE;
      uint32_t* tile = bufs.get<uint32_t>(2 * n_tiles); uint32_t* totals = bufs.get<uint32_t>(2);
      tasks[k].off = bufs.get<uint32_t>(2 * n);
      hip_check(mkp_launch_dmr_reps_tasks(st, outs[k].present, joined[k].n, rep_stride, tile, totals, tasks[k].off), "dmr replicates tasks launch");
      d2h_copy(tasks[k].n, totals, 8, st);
    }
    D.stage_ms[5] = ms_between(clk);
    for (size_t k = 0; k < nt; k++)
      hip_check(mkp_launch_dmr_reps_score(st, tasks[k].off, tasks[k].n[0], tasks[k].n[1], joined[k].n, nc, rep_stride, &math, &outs[k]),
          "dmr replicates score launch");
    hip_check(hipStreamSynchronize(st), "dmr replicates score sync");
    D.stage_ms[6] = ms_between(clk);

    // ---- read-back, and the written sites in walk order
    uint64_t n_all = 0; for (const Joined& J : joined) n_all += J.n;
    D.h_tid.clear(); D.h_pos.clear(); D.h_strand.clear(); D.h_score.clear(); D.h_p.clear(); D.h_effect.clear(); D.h_bal_p.clear(); D.h_bal_effect.clear();
    D.h_rep_p.clear(); D.h_rep_effect.clear(); D.h_n_rep.clear();
    for (int s = 0; s < 2; s++) { D.h_total[s].clear(); D.h_mod[s].clear(); D.h_has[s].clear(); D.h_pct[s].clear(); }
    D.h_tid.reserve(n_all); D.h_pos.reserve(n_all); D.h_score.reserve(n_all);
    uint64_t n_failed = 0; double read_ms = 0;
    std::vector<uint32_t> pos, info, has, pct, tot, cnt, n_rep; std::vector<double> score, pv, eff, bpv, beff, rpv, reff;
    for (size_t k = 0; k < nt; k++) {
      const size_t n = joined[k].n; const MkpDmrRepsSites& O = outs[k];
      auto t_read = std::chrono::steady_clock::now();
      pos.resize(n); info.resize(n); has.resize(n); pct.resize(n); tot.resize(2 * n); cnt.resize(n * 2 * nc); n_rep.resize(n); score.resize(n); pv.resize(n);
      eff.resize(n); bpv.resize(n); beff.resize(n); rpv.resize(n * rep_stride); reff.resize(n * rep_stride);
      d2h_copy(pos.data(), O.pos, n * 4, st); d2h_copy(info.data(), O.info, n * 4, st); d2h_copy(has.data(), O.has, n * 4, st);
      d2h_copy(pct.data(), O.pct, n * 4, st); d2h_copy(tot.data(), O.total, n * 8, st); d2h_copy(cnt.data(), O.cnt, n * 2 * nc * 4, st);
      d2h_copy(n_rep.data(), O.n_rep, n * 4, st); d2h_copy(score.data(), O.score, n * 8, st); d2h_copy(pv.data(), O.pvalue, n * 8, st);
      d2h_copy(eff.data(), O.effect, n * 8, st); d2h_copy(bpv.data(), O.bal_pvalue, n * 8, st); d2h_copy(beff.data(), O.bal_effect, n * 8, st);
      d2h_copy(rpv.data(), O.rep_pvalue, n * rep_stride * 8, st); d2h_copy(reff.data(), O.rep_effect, n * rep_stride * 8, st);
      read_ms += ms_between(t_read);
      for (size_t i = 0; i < n; i++) {
        if (info[i] & MKP_DMRR_SITE_OVERFLOW) throw Error(MKP_E_UNSUPPORTED, "dmr replicates: the summed coverage of " + D.names[tids[k]] + ":"
            + std::to_string(pos[i]) + " does not fit 32 bits");
        if (info[i] & MKP_DMRS_PAIR_FAILED) { n_failed++; continue; }
        D.h_tid.push_back(tids[k]); D.h_pos.push_back(pos[i]); D.h_strand.push_back((info[i] & MKP_DMRS_SITE_MINUS) ? '-' : '+');
        for (int s = 0; s < 2; s++) {
          D.h_total[s].push_back(tot[2 * i + s]); D.h_has[s].push_back(s ? has[i] >> 16 : has[i] & 0xffffu);
          D.h_pct[s].push_back(s ? pct[i] >> 16 : pct[i] & 0xffffu);
          D.h_mod[s].insert(D.h_mod[s].end(), cnt.begin() + (i * 2 + s) * nc, cnt.begin() + (i * 2 + s + 1) * nc);
        }
        D.h_score.push_back(score[i]); D.h_p.push_back(pv[i]); D.h_effect.push_back(eff[i]); D.h_bal_p.push_back(bpv[i]); D.h_bal_effect.push_back(beff[i]);
        D.h_n_rep.push_back(n_rep[i]);
        for (uint32_t r = 0; r < rep_stride; r++) {   // (ranks behind n_rep were never written on the device)
          const bool on = r < n_rep[i];
          D.h_rep_p.push_back(on ? rpv[i * rep_stride + r] : 0.0); D.h_rep_effect.push_back(on ? reff[i * rep_stride + r] : 0.0);
        }
      }
    }
    D.stage_ms[7] = read_ms; D.stage_ms[8] = ms_between(clk) - read_ms;
    memset(out, 0, sizeof(*out));
    mkp_dmr_sites_out& T = out->sites;
    T.n_sites = D.h_pos.size(); T.n_codes = nc; T.code_repr = D.h_codes.data();
    T.tid = D.h_tid.data(); T.pos = D.h_pos.data(); T.strand = D.h_strand.data();
    for (int s = 0; s < 2; s++) { T.total[s] = D.h_total[s].data(); T.n_mod[s] = D.h_mod[s].data(); T.has_code[s] = D.h_has[s].data();
      T.max_coverages[s] = max_cov[s]; T.n_sampled[s] = n_sampled[s]; out->pct_samples[s] = D.h_pct[s].data(); }
    T.score = D.h_score.data(); T.map_pvalue = D.h_p.data(); T.effect_size = D.h_effect.data();
    T.n_batches = n_batches; T.n_batches_dropped = n_dropped; T.n_model_failures = n_failed;
    out->n_a = n_a; out->n_b = n_b; out->balanced_map_pvalue = D.h_bal_p.data(); out->balanced_effect_size = D.h_bal_effect.data();
    out->n_rep = D.h_n_rep.data();
    if (matched) { out->rep_pvalue = D.h_rep_p.data(); out->rep_effect = D.h_rep_effect.data(); }
  });
}

}  // extern "C"
