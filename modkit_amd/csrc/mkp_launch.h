// The seam between the host files and the device objects: every extern "C" entry point a .hip file defines for the host — the kernel
// launchers, the two LDS setters and mkp_merge_tiles — is declared HERE and nowhere else.  The .hip file that defines one includes this
// header, so the compiler checks the definition against the prototype; mkp_api.cpp and mkp_ingest_host.cpp include it to call them.  (C
// linkage keeps parameter types out of the symbol name: a prototype copied by hand into a host file that drifts from its definition still
// links, and passes wrong arguments at run time.)  Adding a launcher: define it in its .hip file, declare it here with every parameter
// named, call it; never write an `extern "C"` prototype into a .cpp file (tests/test_launch_header_host.py looks for those).
#pragma once
#include <hip/hip_runtime_api.h>

#include "mkp_device.h"
#include "mkp_dmr_site_math.hpp"

// mkp_ingest_dev.hpp (the ingest launchers take these by pointer only; the header itself stays out of the other translation units)
struct MkpZChain; struct MkpZBlk; struct MkpSeg; struct MkpIngestParams; struct MkpIngestTotals; struct MkpRecInfo; struct MkpRecDigest;

// The arrays of a packed shard in HBM (layout: mkp_device.h), as the decode, hemi, name-sharing, slot, tile and sampling launchers take them.
// Host side only: a launcher unpacks it into its kernels' argument lists, it is never a kernel argument itself.
struct MkpShardArrays {
  MkpReadHdr* hdr;             // (mkp_dup_restore / mkp_dup_apply move a consumer's event slice in and out of its header)
  const uint32_t* cigar;
  const uint16_t* cigar16;
  const uint32_t* chunk_pfx;   // {query offset, reference offset} pairs: two dwords per entry
  const uint8_t* seq;
  const MkpTagRef* tagref;
  const uint32_t* ranks;
  const uint8_t* ml;
  const MkpLayout* layouts;
  MkpEvent* events;
  MkpReadOut* readout;
};

// The pass words: the 64-byte header in front of the look-back words (slot pipeline) or the tiles' row offsets (tile pipeline) of a pileup
// pass, indices of dwords.  One memset readies header and look-back words together; the host reads the first four words back after a pass.
// The error word holds the ERR_* bits of mkp_device.h.  A sampling pass keeps the same three words in a buffer of its own.
enum : uint32_t {
  MKP_PW_CURSOR = 0,      // row cursor of the accumulate kernels / tile ticket of mkp_pileup_stream
  MKP_PW_ROW_TOTAL = 1,   // rows of the pass (written by the gather, or by the last run of mkp_pileup_stream)
  MKP_PW_ERR = 2,         // error word
  MKP_PW_RUNS = 16,       // first look-back word / row offset
  MKP_PW_HEADER_BYTES = 4 * MKP_PW_RUNS
};

extern "C" {

// ---- mkp_kernels.hip: event decoders, tile pipeline, sampling
// read_ids: read ids by decode class, n_class[7] lists of them one behind the other; prm: host copy (passed to the kernels by value);
// bedmask: the focus bytes of a pileup pass or the --include-bed mask of a sampling pass; sample_vals: sampling passes only
hipError_t mkp_launch_decode(hipStream_t st, const MkpShardArrays& sh, const uint32_t* read_ids, const uint32_t* n_class /* [7] */,
    const MkpRunParams* prm, uint32_t* dev_err, const uint8_t* bedmask, float* sample_vals);
hipError_t mkp_pileup_set_lds(uint32_t accum_bytes);
// hemi: pileup-hemi (slotbm = the run's slot bitmap, otherwise unused); prm_dev: device copy; tile_row_off / tile_row_cnt: one word per
// (key pass, tile); key_slot: index of the key pass
hipError_t mkp_launch_pileup(hipStream_t st, uint32_t lds_bytes, bool hemi, const MkpShardArrays& sh, const MkpTile* tiles, uint32_t n_tiles,
    const MkpRunParams* prm_dev, const uint32_t* slotbm, const MkpRowsDev* rows, uint32_t* row_cursor, uint32_t* tile_row_off,
    uint32_t* tile_row_cnt, uint32_t* dev_err, uint32_t key_filter, uint32_t key_slot, bool wide);
// iv_start: the n_iv interval starts of the reference's grid
hipError_t mkp_launch_hemi_failed(hipStream_t st, const MkpShardArrays& sh, uint32_t n_reads, const uint32_t* slotbm, const uint32_t* iv_start,
    uint32_t n_iv, int32_t win_start, int32_t win_end, uint32_t* dev_err);
// n_tiles: row runs (key passes x tiles); src -> dst: the runs' rows into genome order, *total_rows of them
hipError_t mkp_launch_gather(hipStream_t st, const uint32_t* tile_row_off, const uint32_t* tile_row_cnt, uint32_t* tile_dst_off, uint32_t n_tiles,
    uint32_t* total_rows, const MkpRowsDev* src, const MkpRowsDev* dst);
// take: one byte per read of the last sampling pass; store: the resident sample (store_cap values), hist0: its level-0 histograms
hipError_t mkp_launch_sample_accumulate(hipStream_t st, const MkpShardArrays& sh, const uint8_t* take, uint32_t n_reads, const float* vals,
    uint32_t* store, unsigned long long store_cap, unsigned long long* store_cursor, uint32_t* hist0, uint32_t* dev_err);
hipError_t mkp_launch_sample_hist1(hipStream_t st, const uint32_t* store, unsigned long long n, uint32_t base, uint32_t prefix, uint32_t* hist1);
// table: 128 call counters, reads_with: 6 per-read counters
hipError_t mkp_launch_summary_accumulate(hipStream_t st, const MkpShardArrays& sh, const uint8_t* take, uint32_t n_reads,
    unsigned long long* table, unsigned long long* reads_with);

// ---- mkp_slots.hip: slot pipeline, records sharing a read name
// work: the fused decoder's reads (longest first); call_plane / base_plane: their two planes, MkpWork.pad indexes both; cover_ids: the reads
// of mkp_cover_reads; prm: host copy; cov: the feature stream
hipError_t mkp_launch_slots(hipStream_t st, const MkpWork* work, uint32_t n_fused, const MkpCallEnt* call_plane, const MkpBaseEnt* base_plane,
    const MkpShardArrays& sh, const uint32_t* cover_ids, uint32_t n_cover, const MkpFusedDesc* fdesc, const MkpRunParams* prm,
    const uint32_t* slot_pos, const MkpSlotEnt* slot_ent, uint8_t* cov, MkpVisit* visits);
// seqn_bytes: += the SEQ bytes the decoder reads of MKP_RF_SEQN reads
hipError_t mkp_launch_call_plane(hipStream_t st, MkpWork* work, uint32_t n_fused, const MkpShardArrays& sh, const MkpFusedDesc* fdesc,
    MkpCallEnt* call_plane, MkpBaseEnt* base_plane, unsigned long long* seqn_bytes);
hipError_t mkp_stream_set_lds(uint32_t bytes);
hipError_t mkp_launch_dup_restore(hipStream_t st, const MkpShardArrays& sh, const MkpDupCons* cons, uint32_t n);
hipError_t mkp_launch_dup_events(hipStream_t st, const MkpShardArrays& sh, MkpDupCons* cons, const MkpDupSeg* segs, uint32_t n, uint32_t* dev_err);
// prm_dev: device copy; tile_row_off: the look-back words, n_runs of them (row runs of the launch sequence: key passes x tiles); key_slot:
// index of the key pass; n_combos: motif combos; slot_cap: slot capacity of a tile; words_per_slot: tally words per slot
hipError_t mkp_launch_stream(hipStream_t st, uint32_t lds_bytes, const MkpVisit* visits, const uint8_t* cov, const MkpEvent* events,
    const MkpSTile* tiles, uint32_t n_tiles, const MkpRunParams* prm_dev, const uint32_t* slot_pos, const uint8_t* focus, const MkpCombo* combos,
    const MkpRowsDev* rows, uint32_t* row_cursor, uint32_t* tile_row_off, uint32_t* dev_err, uint32_t key_filter, uint32_t key_slot,
    uint32_t n_combos, uint32_t n_runs, uint32_t slot_cap, uint32_t words_per_slot, bool wide);

// ---- mkp_inflate_wave4.hip.  variant: ring size in KiB, 8 or 2; anything else = the 4 KiB kernel
hipError_t mkp_launch_inflate_wave4(hipStream_t st, const uint8_t* in, const MkpBgzfBlock* blocks, uint32_t n_blocks, uint8_t* out,
    uint32_t* status, int variant);

// ---- mkp_ingest.hip
hipError_t mkp_launch_widen(hipStream_t st, const uint32_t* in, unsigned long long* out, uint32_t n);
hipError_t mkp_launch_bgzf_chain_count(hipStream_t st, const uint8_t* z, const MkpZChain* chains, uint32_t n, uint32_t* cnt, uint32_t* err);
hipError_t mkp_launch_bgzf_chain_write(hipStream_t st, const uint8_t* z, const MkpZChain* chains, uint32_t n, const uint32_t* base, uint32_t cap,
    MkpZBlk* out, uint32_t* err);
hipError_t mkp_launch_bgzf_layout(hipStream_t st, const MkpZBlk* zb, uint32_t n, unsigned long long* raw_cursor, unsigned long long raw_cap,
    MkpBgzfBlock* out, uint32_t* err);
hipError_t mkp_launch_crc32(hipStream_t st, const uint8_t* zin, const MkpBgzfBlock* blocks, uint32_t n_blocks, const uint8_t* raw,
    uint32_t* status);
hipError_t mkp_launch_ingest_count(hipStream_t st, const uint8_t* raw, const MkpIngestParams* P, const MkpSeg* segs, uint32_t* seg_cnt,
    MkpIngestTotals* tot);
hipError_t mkp_launch_ingest_parse(hipStream_t st, const uint8_t* raw, const MkpIngestParams* P, const int32_t* parts, const MkpSeg* segs,
    const uint32_t* seg_base, unsigned long long* rec_off, MkpRecInfo* info, uint32_t* sz, int32_t* extra, MkpIngestTotals* tot);
hipError_t mkp_launch_ingest_pack(hipStream_t st, const uint8_t* raw, uint32_t rec_cap, const MkpRecInfo* info, const uint32_t* sz, MkpReadHdr* hdr,
    uint32_t* cigar, uint16_t* cigar16, uint32_t* chunk_pfx, uint8_t* seq, MkpTagRef* tagref, uint32_t* ranks, uint8_t* ml, MkpRecDigest* dig,
    MkpIngestTotals* tot);

// ---- mkp_stats.hip, mkp_dmr.hip, mkp_localize.hip: pos .. n_mod are row columns, n_rows rows; row_lo / row_hi: first row of a region and the row behind
// its last; ev: 3 timing events or NULL
// n_chunks / off / total: chunks per region, their offsets and total; out: the run's table, seen: its masks, codes: its slot codes;
// min_cov: least coverage of a counted row; fixed_codes: the code list is fixed
hipError_t mkp_launch_region_stats(hipStream_t st, const uint32_t* pos, const uint32_t* info, const uint32_t* code, const uint32_t* n_valid,
    const uint32_t* n_mod, uint32_t n_rows, const MkpStatsRegion* regions, uint32_t n_regions, uint32_t* row_lo, uint32_t* row_hi, uint32_t* n_chunks,
    unsigned long long* off, unsigned long long* total, unsigned long long* out, uint32_t* seen, uint32_t* codes, uint32_t* err,
    unsigned long long min_cov, uint32_t fixed_codes, hipEvent_t* ev);
// mkp_dmr.hip: as mkp_launch_region_stats, with the n_canonical column; ref: the contig's reference bytes [ref_off, ref_off + ref_len) (NULL
// with ref_len 0: no position has a base); prm: host copy; out / seen: ONE sample's lines of the run's table
hipError_t mkp_launch_dmr(hipStream_t st, const uint32_t* pos, const uint32_t* info, const uint32_t* code, const uint32_t* n_valid,
    const uint32_t* n_mod, const uint32_t* n_can, uint32_t n_rows, const MkpStatsRegion* regions, uint32_t n_regions, uint32_t* row_lo,
    uint32_t* row_hi, uint32_t* n_chunks, unsigned long long* off, unsigned long long* total, const uint8_t* ref, uint32_t ref_off, uint32_t ref_len,
    const MkpDmrParams* prm, unsigned long long* out, uint32_t* seen, uint32_t* codes, uint32_t* err, hipEvent_t* ev);
// tab: the run's table, codes: its slot codes
hipError_t mkp_launch_localize(hipStream_t st, const uint32_t* pos, const uint32_t* info, const uint32_t* code, const uint32_t* n_valid,
    const uint32_t* n_mod, uint32_t n_rows, const MkpLocRegion* regions, uint32_t n_regions, uint32_t* row_lo, uint32_t* row_hi, uint32_t window,
    uint32_t stranded, unsigned long long* tab, uint32_t* codes, uint32_t* err, hipEvent_t* ev);

// ---- mkp_dmr_sites.hip: the rows of ONE contig of one sample (pos .. n_can: row columns, n_rows rows), the contig's reference bytes [0, ref_len)
// counts: n_windows words, the listed positions per window of `interval` bp
hipError_t mkp_launch_dmr_sites_listed(hipStream_t st, const uint8_t* ref, uint32_t ref_len, unsigned long long interval, uint32_t n_windows,
    const MkpDmrParams* prm, uint32_t* counts);
// flags + scan + heads.  codes / err: the run's slot codes and error word; rowflag: a byte a row; tile_cnt: two words per tile of MKP_DMRS_TILE
// rows, left as the exclusive prefixes of heads and participating rows; totals: two words, sites and participating rows; s_*: the sites
hipError_t mkp_launch_dmr_sites_heads(hipStream_t st, const uint32_t* pos, const uint32_t* info, const uint32_t* code, const uint32_t* n_valid,
    const uint32_t* n_mod, const uint32_t* n_can, uint32_t n_rows, const uint8_t* ref, uint32_t ref_len, const MkpDmrParams* prm, uint32_t* codes,
    uint32_t* err, uint8_t* rowflag, uint32_t* tile_cnt, uint32_t* totals, uint32_t* s_pos, uint32_t* s_first, uint32_t* s_total, uint32_t* s_info);
// per entry of the contig's batch table: the first row at or behind its start, and the participating rows in front of that row
hipError_t mkp_launch_dmr_sites_bounds(hipStream_t st, const uint32_t* pos, const uint8_t* rowflag, uint32_t n_rows, const uint32_t* tile_off,
    const uint32_t* totals, const MkpDmrSitesBatch* batches, uint32_t n_entries, uint32_t* row_at, uint32_t* part_before);
// out[*cursor ++] = N_valid_cov of every participating row among the first n_front (any order; a value past `cap` is dropped)
hipError_t mkp_launch_dmr_sites_coverages(hipStream_t st, const uint8_t* rowflag, const uint32_t* n_valid, uint32_t n_front, uint32_t* cursor,
    uint32_t* out, uint32_t cap);
// bad_batch: a word per batch of the run, set by a bad site of either sample
hipError_t mkp_launch_dmr_sites_bad(hipStream_t st, const uint32_t* s_pos, const uint32_t* s_info, uint32_t n_sites, const MkpDmrSitesBatch* batches,
    uint32_t n_entries, uint32_t* bad_batch);
// join + scan + pairs.  partner: n_a words; tile_cnt: two words per tile of a's sites; totals[0]: the pairs; pair_a / pair_b: site indices
hipError_t mkp_launch_dmr_sites_join(hipStream_t st, const uint32_t* a_pos, uint32_t n_a, const uint32_t* b_pos, uint32_t n_b,
    const MkpDmrSitesBatch* batches, uint32_t n_entries, const uint32_t* bad_batch, uint32_t* partner, uint32_t* tile_cnt, uint32_t* totals,
    uint32_t* pair_a, uint32_t* pair_b);
// col_of_slot: 4 bits a slot, its code column (columns ascend in code); a, b, math, out: host copies
hipError_t mkp_launch_dmr_sites_score(hipStream_t st, const MkpDmrSitesSample* a, const MkpDmrSitesSample* b, const uint32_t* pair_a,
    const uint32_t* pair_b, uint32_t n_pairs, unsigned long long col_of_slot, uint32_t n_cols, const MkpDmrSiteMath* math, const MkpDmrSitesPairs* out);

// the scan alone: cnt = two counters per tile -> their exclusive prefixes, totals[0 .. 2) = the sums
hipError_t mkp_launch_dmr_sites_scan(hipStream_t st, uint32_t* cnt, uint32_t n_tiles, uint32_t* totals);

// ---- mkp_dmr_reps.hip: ONE contig; bits: a side's site bitmap, n_words words of 32 positions, zeroed by the caller
hipError_t mkp_launch_dmr_reps_mark(hipStream_t st, const uint32_t* s_pos, uint32_t n_sites, uint32_t* bits, uint32_t n_words);
// join + scan.  a_bits is left as the joined bitmap; tile_cnt: two words per tile of MKP_DMRS_TILE words, left as exclusive prefixes;
// totals[0]: the joined sites
hipError_t mkp_launch_dmr_reps_join(hipStream_t st, uint32_t* a_bits, const uint32_t* b_bits, uint32_t n_words, const MkpDmrSitesBatch* batches,
    uint32_t n_entries, const uint32_t* bad_batch, uint32_t* tile_cnt, uint32_t* totals);
// j_pos: the n_joined joined positions, ascending
hipError_t mkp_launch_dmr_reps_list(hipStream_t st, const uint32_t* bits, uint32_t n_words, const uint32_t* tile_off, uint32_t* j_pos, uint32_t n_joined);
// samples: DEVICE array, the n_a samples of a then the n_b of b; rep_stride: the samples a side of a matched run, otherwise 0; out: host copy
hipError_t mkp_launch_dmr_reps_gather(hipStream_t st, const MkpDmrRepsSample* samples, uint32_t n_a, uint32_t n_b, const uint32_t* j_pos,
    uint32_t n_joined, unsigned long long col_of_slot, uint32_t n_cols, uint32_t rep_stride, const MkpDmrRepsSites* out);
// count + scan + first tasks.  present: the joined sites' presence masks; tile_cnt: two words per tile of MKP_DMRS_TILE sites; totals[0 .. 2):
// the p-value tasks and the ratio tasks; task_off[2 * site + {0, 1}]: the site's first task of either kind
hipError_t mkp_launch_dmr_reps_tasks(hipStream_t st, const uint32_t* present, uint32_t n_joined, uint32_t rep_stride, uint32_t* tile_cnt,
    uint32_t* totals, uint32_t* task_off);
// the p-value kernel over its tasks, then the ratio kernel over its own
hipError_t mkp_launch_dmr_reps_score(hipStream_t st, const uint32_t* task_off, uint32_t n_pmap_tasks, uint32_t n_ratio_tasks, uint32_t n_joined,
    uint32_t n_cols, uint32_t rep_stride, const MkpDmrSiteMath* math, const MkpDmrRepsSites* out);

// ---- mkp_merge.hip.  a: the table, b: the added rows, stage: staging, out: the new table, *n_out its rows; cuts: mkp_merge_tiles(n_a + n_b) + 1
// entries, counts / offsets: mkp_merge_tiles(n_a + n_b) each; ev: 3 timing events or NULL
hipError_t mkp_launch_merge(hipStream_t st, const MkpRowsDev* a, uint32_t n_a, const MkpRowsDev* b, uint32_t n_b, const MkpRowsDev* stage,
    const MkpRowsDev* out, MkpMergeCut* cuts, uint32_t* counts, uint32_t* offsets, uint32_t* n_out, uint32_t* err, hipEvent_t* ev);
// *out = rows with pos < limit
hipError_t mkp_launch_merge_rows_below(hipStream_t st, const uint32_t* pos, uint32_t n, uint32_t limit, uint32_t* out);
uint32_t mkp_merge_tiles(uint64_t n_rows);

// ---- mkp_bedmethyl.hip.  text: n > 0 bytes of bedMethyl text, the buffer reaching to the next multiple of MKP_BEDIN_CHUNK; words: the piece's
// MKP_BEDIN_WORDS words (mkp_device.h), zeroed, MKP_BEDIN_W_ERR_OFF set to all ones; final_piece: a last line without '\n' is a line
// count + scan: cnt = three words per chunk, the first n_chunks left as the chunks' first data lines; the host reads the words next
hipError_t mkp_launch_bedmethyl_lines(hipStream_t st, const uint8_t* text, uint32_t n, uint32_t final_piece, uint32_t* cnt, uint32_t* words);
// line starts + parse + runs.  n_lines / n_rows / limit: as read from the words; chunk_off: the cnt of the call above; line_start: n_lines + 1
// words; rows: n_rows rows a column; runs: n_rows entries, names: n bytes (both in the order the runs were met, not file order); max_line: a
// longer line (without its '\n') sets MKP_BEDIN_ERR_LONG
hipError_t mkp_launch_bedmethyl_parse(hipStream_t st, const uint8_t* text, uint32_t n, uint32_t n_lines, uint32_t n_rows, uint32_t limit,
    uint32_t max_line, const uint32_t* chunk_off, uint32_t* line_start, const MkpRowsDev* rows, MkpBedRun* runs, uint8_t* names, uint32_t* words);

}  // extern "C"
