/* mkpileup.h — C ABI of libmkpileup: the MI355X (gfx950) implementation of modkit's `pileup`
 * hot path (MM/ML decode -> threshold caller -> per-position aggregation -> bedMethyl rows).
 *
 * The reference (nanoporetech/modkit v0.4.4, pure Rust) has no FFI on this path.  The seam this
 * library replaces is the Rust function
 *     pub fn process_region_batch(&MultiChromCoordinates, bam_fp, &MultipleThresholdModCaller,
 *                                 &PileupNumericOptions, force_allow, combine_strands, max_depth,
 *                                 Option<&EdgeFilter>, Option<&Vec<SamTag>>)
 *         -> Vec<Result<ModBasePileup, String>>                       (src/pileup/mod.rs:684-716)
 * called from ModBamPileup::run (src/pileup/subcommand.rs:733-753) and consumed by
 * PileupWriter::write (src/writers.rs:159-183).  Each entry point below names the reference item
 * it stands in for.  INTEGRATION.md shows the Rust `extern "C"` binding.
 *
 * Conventions: every function returns MKP_OK (0) or a negative mkp_status and never unwinds;
 * mkp_last_error() gives the message.  A mkp_ctx is NOT thread-safe (one per host worker thread,
 * any number per GPU).  Input buffers stay owned by the caller and may be freed as soon as the
 * call that read them returns.  Output arrays (mkp_rows) are owned by the ctx and stay valid
 * until the next mkp_shard_run/mkp_process_region on that ctx or mkp_ctx_destroy.
 * There is no CPU fallback: inputs the device path does not cover fail with MKP_E_UNSUPPORTED.
 */
#ifndef MKPILEUP_H
#define MKPILEUP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MKP_OK = 0,
  MKP_E_INVALID = -1,     /* bad argument / call order */
  MKP_E_IO = -2,          /* file open / parse failure */
  MKP_E_UNSUPPORTED = -3, /* input outside the device path's coverage */
  MKP_E_DEVICE = -4,      /* HIP runtime error, or no gfx950 device */
  MKP_E_NOMEM = -5,
  MKP_E_THRESHOLD = -6    /* threshold estimation failed (e.g. < 2 datapoints, thresholds.rs:18) */
} mkp_status;

typedef struct mkp_ctx mkp_ctx;

typedef struct {
  int32_t device;          /* HIP device ordinal */
  uint32_t tile_positions; /* reference positions per LDS tile; 0 = derive from the LDS budget */
  uint32_t reserved[6];
} mkp_config;

/* mod code encoding = ModCodeRepr (src/mod_base_code.rs:105-109):
 *   Code(char)  -> the code point (e.g. 'm' = 0x6d);  ChEbi(id) -> 0x80000000 | id.
 * Numeric order of this encoding is the reference's row order (derived Ord: Code < ChEbi). */
#define MKP_CODE_CHAR(c) ((uint32_t)(unsigned char)(c))
#define MKP_CODE_CHEBI(id) (0x80000000u | (uint32_t)(id))

typedef struct { uint32_t code_repr; float threshold; } mkp_mod_threshold;

/* Replaces MultipleThresholdModCaller (src/threshold_mod_caller.rs:8-13) + PileupNumericOptions
 * (src/pileup/mod.rs:667-671) + EdgeFilter (src/mod_bam.rs:1634-1639) + the force_allow /
 * combine_strands / max_depth arguments of process_region_batch. Bases are indexed A,C,G,T = 0..3. */
typedef struct {
  float default_threshold;
  float per_base_threshold[4];
  uint8_t has_per_base[4];
  const mkp_mod_threshold* per_mod;
  uint32_t n_per_mod;
  uint32_t numeric_mode;   /* 0 Passthrough, 1 Combine (--combine-mods), 2 Collapse(ReDistribute(collapse_code)) */
  uint32_t collapse_code;  /* code_repr, used when numeric_mode == 2 (--ignore / --preset traditional) */
  uint32_t edge_filter;    /* 0/1 */
  uint32_t edge_start, edge_end, edge_inverted;
  uint32_t force_allow_implicit;
  uint32_t combine_strands;
  uint32_t max_depth;      /* htslib's maxcnt: a shard in which bam_plp_push would drop a record under this cap fails loudly */
} mkp_caller;

/* One alignment record = the fields of htslib's bam1_t the path reads
 * (rust-htslib Record: tid/pos/flags/cigar/seq/aux — src/pileup/mod.rs:783-862, src/mod_bam.rs:1388-1470).
 * `data` is bam1_t::data: qname | cigar u32[n_cigar] | 4-bit seq | qual | aux. */
typedef struct {
  int32_t tid;
  int32_t pos;
  uint16_t flag;
  uint16_t l_qname; /* including the NUL, as bam1_core_t.l_qname */
  uint32_t n_cigar;
  int32_t l_qseq;
  int32_t l_data;
  const uint8_t* data;
} mkp_record;

/* Focus positions of a shard = FocusPositions (src/interval_chunks.rs:32-59) flattened:
 * one byte per reference position of [start,end): bits 0-1 = strand rule (1 = '+' tally only,
 * 2 = '-' tally only, 3 = both, 0 = position not in focus); bits 2-7 = index into `combos`
 * (0 = no motif ids).  focus == NULL means FocusPositions::AllPositions. */
#define MKP_MAX_MOTIF_IDS 4
typedef struct {
  uint8_t n_pos;                          /* motif ids attached to '+' rows (get_positive_strand_motif_ids) */
  uint8_t n_neg;                          /* motif ids attached to '-' rows (get_negative_strand_motif_ids) */
  uint8_t pos_ids[MKP_MAX_MOTIF_IDS];
  uint8_t neg_ids[MKP_MAX_MOTIF_IDS];
  int8_t pos_delta[MKP_MAX_MOTIF_IDS];    /* combine-strands: MotifInfo::negative_strand_position offset; -128 = none */
  uint8_t pad[2];
} mkp_motif_combo;

typedef struct {
  int32_t tid;
  uint32_t start, end;          /* reference window; rows are produced for positions in [start,end) */
  const uint8_t* focus;         /* (end-start) bytes or NULL */
  const mkp_motif_combo* combos;
  uint32_t n_combos;
} mkp_shard;

/* Result rows = PileupFeatureCounts (src/pileup/mod.rs:54-68) as SoA, already in the order
 * ModBasePileup::iter_counts_sorted + the per-position (strand, code) sort would give
 * (src/pileup/mod.rs:440-443, 659-664).  fraction_modified is n_mod as f32 / n_valid as f32. */
typedef struct {
  uint64_t n_rows;
  const uint32_t* pos;
  const uint8_t* strand;      /* '+', '-' or '.' */
  const uint32_t* code_repr;
  const int32_t* motif_idx;   /* -1 = None */
  const uint32_t* n_valid;    /* filtered_coverage */
  const uint32_t* n_mod;
  const uint32_t* n_canonical;
  const uint32_t* n_other;
  const uint32_t* n_delete;
  const uint32_t* n_fail;     /* n_filtered */
  const uint32_t* n_diff;
  const uint32_t* n_nocall;
  /* Log-only counters (the reference prints them at debug level).  Here: kept records of the SHARD whose tags yielded calls /
   * that only contribute coverage.  The reference counts per INTERVAL cache, distinct read names (read_cache.rs:357-365): a read
   * spanning k intervals is counted k times there, once here; the sums over a run differ, the rows do not. */
  uint64_t processed_records;
  uint64_t skipped_records;
  /* --partition-tag (PartitionKey, src/pileup/mod.rs:607-610, 795-815): rows are grouped by key (all rows of key 0, then key 1, ..),
   * genome order inside a key.  partition_key[i] indexes partition_key_names; name 0 is "ungrouped" (PartitionKey::NoKey: no
   * partition tags set, or the read carries none of them); the others are the tag values joined by '_' ("missing" for an absent
   * tag), which is the file stem PartitioningBedMethylWriter uses (src/writers.rs:1029-1080). */
  const uint32_t* partition_key;
  uint32_t n_partition_keys;
  const char* const* partition_key_names;
} mkp_rows;

typedef struct {
  double pack_ms, h2d_ms, kernel_ms, d2h_ms;  /* last shard */
  double decode_kernel_ms, pileup_kernel_ms, gather_kernel_ms;
  uint64_t n_reads, n_events, n_rows, n_tiles, n_positions;
  uint64_t alg_bytes_decode, alg_bytes_pileup; /* SURVEY.md §8(d) algorithmic bytes of the decode and pileup kernels */
  double rows_kernel_ms; /* always 0: rows are emitted by the aggregation kernels straight from LDS (kept for layout compatibility) */
  uint64_t alg_bytes_rows;                     /* 44 B per row */
  /* focus runs on the slot pipeline: feature-stream bytes (one per read and focus position in its span) and
   * SURVEY §8(d)'s literal B_agg = 8 B per coverage / call event + 44 B per row for the aggregation kernel */
  uint64_t stream_bytes, alg_bytes_agg_survey;
  uint32_t slot_pipeline, reserved;
} mkp_stats;

/* ---- lifecycle */
int mkp_ctx_create(const mkp_config* cfg, mkp_ctx** out);
void mkp_ctx_destroy(mkp_ctx* ctx);
const char* mkp_last_error(const mkp_ctx* ctx);
const char* mkp_version(void);
/* ABI revision of THIS header: bumped whenever a struct the caller allocates changes size or layout (mkp_run_report grew in round 5:
 * revision 2; round 6 = 3).  The library writes whole structs of its own revision, so a caller built against another header must not
 * hand it its structs: compare once at start-up —  `mkp_abi_version() == MKP_ABI_VERSION && mkp_run_report_size() == sizeof(mkp_run_report)`
 * (the Rust binding asserts the same on its #[repr(C)] mirror). */
#define MKP_ABI_VERSION 5u
uint32_t mkp_abi_version(void);
size_t mkp_run_report_size(void);
/* Threads of the library's host pool (BGZF inflate, packing, planning, text): the CPUs this process may use — affinity mask and
   cgroup CPU quota — capped at 64; MKP_POOL_THREADS in the environment overrides it.  Rayon's `-t` in the reference
   (subcommand.rs:486-489) is the matching knob. */
unsigned mkp_host_threads(void);

/* ---- caller / options: stands in for the `caller`, `pileup_numeric_options`, `force_allow`,
 *      `combine_strands`, `max_depth`, `edge_filter` arguments of process_region_batch */
int mkp_set_caller(mkp_ctx* ctx, const mkp_caller* caller);

/* ---- partition tags: the `partition_tags: Option<&Vec<SamTag>>` argument of process_region_batch (src/pileup/mod.rs:693).
 * tags = two-character SAM tag names (e.g. "HP", "RG"); n = 0 clears.  Applies to the shards begun afterwards. */
int mkp_set_partition_tags(mkp_ctx* ctx, const char* const* tags, uint32_t n);

/* ---- the hot path on records the host already holds (rust-htslib fetch()+records()):
 * begin a shard, append its records in coordinate order, run.  Replaces the body of
 * process_region (src/pileup/mod.rs:718-1020) for every interval inside the shard. */
int mkp_shard_begin(mkp_ctx* ctx, const mkp_shard* shard);
int mkp_shard_add_records(mkp_ctx* ctx, const mkp_record* recs, uint32_t n);
/* Optional, between begin and run: the ascending start positions of the reference's intervals inside the shard (the last one ends with
 * the window).  The reference keeps one read cache per interval, keyed by read NAME (src/read_cache.rs:28-35): two kept records with one
 * name interfere only when they overlap a common interval — there the record asked about first owns the name and the later ones are
 * answered from its calls (get_mod_call, src/read_cache.rs:232-297), which the library reproduces (round 6; refused before); mates / split
 * alignments lying in different intervals are independent reads.  Without this call the whole shard counts as one interval.  Still
 * MKP_E_UNSUPPORTED: pileup-hemi with such records, and a record whose owners in different intervals disagree in status or codes. */
int mkp_shard_set_intervals(mkp_ctx* ctx, const uint32_t* interval_starts, uint32_t n_intervals);
int mkp_shard_run(mkp_ctx* ctx, mkp_rows* out);

/* ---- the same seam one level up: process_region_batch(&MultiChromCoordinates, ...) (src/pileup/mod.rs:684-716, called per batch from
 * ModBamPileup::run, src/pileup/subcommand.rs:733-753) in ONE call.  intervals = the batch's ChromCoordinates (each a mkp_shard: window +
 * focus bytes of that interval), in the order the feeder produced them; recs = the records the caller fetched for the batch — every
 * record overlapping any of the intervals once, coordinate order per contig.  Intervals that follow each other on one contig
 * (start == previous end, same kind of focus, same combo table) are merged into ONE resident shard — one pack, one plan, one launch
 * sequence, one read-back instead of one per interval — and cut apart again at their ends: out[k] = the rows of intervals[k], arrays
 * owned by the ctx until its next run.  processed / skipped_records are reported on the first interval of each merged run.  With
 * partition tags set every interval runs alone (its rows come grouped by key).  Per-interval calls cost ~1.7 ms of launch and planning
 * latency each (bench.py: tiers.seam_per_interval); a batch pays it once per contig run. */
int mkp_batch_run(mkp_ctx* ctx, const mkp_shard* intervals, uint32_t n_intervals, const mkp_record* recs, uint32_t n_recs, mkp_rows* out);

/* Re-run the device pipeline on the shard that is already resident in HBM (no pack, no H2D):
 * what bench.py times.  `iters` launches; rows of the last one are returned. */
int mkp_shard_rerun(mkp_ctx* ctx, uint32_t iters, mkp_rows* out);
int mkp_get_stats(const mkp_ctx* ctx, mkp_stats* out);
/* DIAGNOSTIC (tests and debugging; no caller needs it to run a pileup, and the bits may grow): what the packer decided per read of the
 * shard that is open or resident, in file order (the reads the pileup keeps): MKP_READ_REVERSE reverse strand, MKP_READ_TAG_ERROR the
 * read only contributes coverage, MKP_READ_WIDE_CIGAR a CIGAR op longer than 4 095 bases — the slot decoder walks the read's 32-bit
 * CIGAR words instead of the 16-bit ones.  *n_reads = reads of the shard; at most `cap` flags are written. */
#define MKP_READ_REVERSE 1u
#define MKP_READ_TAG_ERROR 2u
#define MKP_READ_WIDE_CIGAR 32u
int mkp_shard_read_flags(const mkp_ctx* ctx, uint32_t* flags, uint32_t cap, uint32_t* n_reads);

/* ---- same, reading the BAM itself: direct stand-in for process_region_batch(bam_fp, ...)
 * (src/pileup/mod.rs:684-716; the IndexedReader fetch + pileup of :732-759).  With a .bai next to the file the window's
 * compressed BGZF blocks are uploaded and inflated, cut into records, tokenised and packed ON THE DEVICE: nothing
 * but the index and the block headers is read on the host, and this is the fast seam — the record-level calls above pay the
 * host packer and the upload of packed records.  Without an index (or with partition tags, or MKP_HOST_INGEST=1) the library's
 * host reader + packer feed the same kernels.  One call = one shard: keep the window to ~1 GiB of BAM. */
int mkp_process_region(mkp_ctx* ctx, const char* bam_path, const mkp_shard* shard, mkp_rows* out);

/* ---- whole subcommand: `modkit pileup` (ModBamPileup::run, src/pileup/subcommand.rs:382-816).
 * argv carries the reference's own flags (in.bam out.bed --cpg --ref ... ), see DESIGN.md for the
 * covered set; plus --device N, --gpus-rank R --gpus-world W for interval sharding; plus --region-stats <regions.bed> --region-stats-out
 * <table.tsv> [--region-stats-codes m,h] [--region-stats-min-coverage N] [--region-stats-no-header] [--region-stats-only]: `modkit stats`
 * over the run's rows while they are in HBM (mkp_stats_* below); with --region-stats-only the rows are neither read back nor written
 * (the out.bed positional is still required, the file is not created); plus --localize <regions.bed> --localize-out <table.tsv>
 * [--localize-window N (2000)] [--localize-stranded same|opposite] [--localize-stranded-features +|-|.] [--localize-only]: `modkit localize`
 * over the run's rows (mkp_localize_* below; contig lengths from the BAM header), combinable with --region-stats; plus
 * --merge-bedmethyl <prior.bed> (repeatable): out.bed is `modkit bedmethyl merge` of the run's rows with the prior tables (plain text or bgzip),
 * joined on the device (mkp_merge_* below; contig lengths and order from the BAM header; the run's rows are not read back per shard). */
int mkp_pileup_main(int argc, const char* const* argv, char* errbuf, size_t errbuf_len);

/* The same subcommand on a context the caller owns (so the device named by the ctx is used and --device is ignored):
 * afterwards the last shard is still resident in HBM — mkp_shard_rerun re-launches the kernels on it — and `report`
 * (may be NULL) holds the wall time of every stage of ModBamPileup::run as this library executes it. */
typedef struct {
  double load_ms;       /* BAM open + BGZF inflate + record index (reference: htslib IndexedReader per interval) */
  double threshold_ms;  /* threshold estimation (sampling schedule + device decode of the sampled reads + percentile) */
  double focus_ms;      /* interval grid + motif / BED focus positions (interval_chunks.rs) */
  double pack_ms, h2d_ms, kernel_ms, d2h_ms;   /* summed over shards */
  double write_ms;      /* bedMethyl text + file write the caller waited for */
  double total_ms;
  uint64_t n_rows, n_positions, n_shards, processed_records, skipped_records;
  float threshold[4]; uint8_t has_threshold[4];   /* per-base pass thresholds used (A,C,G,T) */
  /* round 5 — where the wall went that the stages above do not own, so that they add up; and the device ingest's own figures */
  double grid_wait_ms;          /* the threshold estimate waiting for the reference FASTA and the interval grid (not part of threshold_ms) */
  double callback_ms;           /* mkp_pileup_run_cb: inside the caller's threshold callback (all-reduce / broadcast; not part of threshold_ms) */
  double ingest_kernel_ms;      /* device ingest, summed over the shards: the inflate launch + record chains (HIP events) */
  double ingest_upload_ms, ingest_table_ms, ingest_pack_ms;
    /* ... the uploads, the block tables, parse + scans + pack incl. their syncs (host clocks) */
  uint64_t ingest_comp_bytes, ingest_raw_bytes, ingest_blocks, ingest_records;   /* compressed bytes uploaded, bytes they inflated to */
} mkp_run_report;
int mkp_pileup_run(mkp_ctx* ctx, int argc, const char* const* argv, mkp_run_report* report);

/* The same run with the pass thresholds decided by the CALLER at the point where `modkit pileup` estimates them (subcommand.rs:615-638) —
 * the multi-GPU form: every rank calls this with --gpus-rank / --gpus-world and no threshold flags.  The library ingests this rank's shards
 * ahead from the first moment, then calls `fn` once:
 *   have_sample = 1  (`-f 1.0`, thresholds.rs:121-159): the context's histograms hold the sample of THIS rank's shards, taken from HBM;
 *                    the callback sums them over the ranks (mkp_histogram_allreduce, or mkp_histogram_get + its own collective) and
 *                    evaluates the percentile (mkp_histogram_locate / _resolve / mkp_percentile_from_histogram);
 *   have_sample = 0  (the count-based default, `-n`, `-f x < 1`): nothing was sampled — the schedule carries quotas from interval to
 *                    interval and is one rank's job (mkp_estimate_thresholds on a context of its own) — the callback hands over the
 *                    values it received from that rank.
 * The callback fills thresholds[b] / has[b] for b = A, C, G, T and returns MKP_OK; the shards are still resident when it returns and the
 * pileup pass runs on them.  With fn == NULL this is mkp_pileup_run. */
typedef int (*mkp_threshold_fn)(void* user, mkp_ctx* ctx, int have_sample, float thresholds[4], uint8_t has[4]);
int mkp_pileup_run_cb(mkp_ctx* ctx, int argc, const char* const* argv, mkp_threshold_fn fn, void* user, mkp_run_report* report);

/* ---- threshold estimation: get_threshold_from_options (src/command_utils.rs:74-134) ->
 * calc_threshold_from_bam (src/thresholds.rs:121-159).  Which reads are sampled follows the reference's
 * schedule (reads_sampler/, sampling_schedule.rs); their call probabilities are decoded on the GPU.
 * argv = the sampling flags of `modkit pileup` (-n -f -p -t --sampling-interval-size --region --sample-region
 * --include-bed --include-unmapped --edge-filter --ignore --preset). thr/has are indexed A,C,G,T. */
int mkp_estimate_thresholds(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv, float thr[4], uint8_t has[4]);

/* ---- threshold arithmetic: percentile_linear_interp (src/thresholds.rs:17-38) on a sorted array */
int mkp_percentile(const float* sorted, uint64_t n, float q, float* out);

/* ---- the same estimate split for multi-GPU runs: calc_threshold_from_bam (src/thresholds.rs:121-159) sorts the
 * sampled argmax probabilities of each canonical base and interpolates between two order statistics.  Here the sample stays in
 * HBM and is summarised by two-level histograms of the values' f32 bit patterns (positive floats order like unsigned integers):
 * level 0 counts the top 16 bits, level 1 the low 16 bits of the values whose top 16 bits equal `prefix`.  Histograms add, so
 * W ranks that each sampled their own reference windows sum them (ncclAllReduce(sum, u64) over xGMI — the path's one
 * collective) and every rank finds the exact order statistics of the union.  Sequence per rank:
 *   mkp_histogram_begin; mkp_histogram_add_bam(..., "--gpus-rank R --gpus-world W -f 1.0 ...");
 *   per base: get(level 0) -> all-reduce -> mkp_histogram_locate -> get(level 1, bins) -> all-reduce -> mkp_histogram_resolve
 *             -> mkp_percentile_from_histogram.                 (mkp_estimate_thresholds does all of it for one rank.)
 * Histogram arrays are uint64_t[65536]. */
int mkp_histogram_begin(mkp_ctx* ctx);
int mkp_histogram_add_bam(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv);
int mkp_histogram_get(mkp_ctx* ctx, uint32_t base /*A,C,G,T = 0..3*/, uint32_t level, uint32_t prefix, uint64_t* out);
/* mkp_histogram_get + the all-reduce in one call, on the device: the histogram is widened to u64 in HBM and summed over the ranks of
 * `nccl_comm` (an ncclComm_t the caller created with ncclCommInitRank, one rank per GPU) with ncclAllReduce(ncclUint64, ncclSum) over
 * xGMI on the context's stream; `out` receives the sum.  Every rank must make the same calls in the same order.  librccl.so is loaded
 * at run time.  (modkit_amd.distributed uses it when the job runs on the nccl backend; torch.distributed's all_reduce is the test
 * double on gloo.) */
int mkp_histogram_allreduce(mkp_ctx* ctx, void* nccl_comm, uint32_t base, uint32_t level, uint32_t prefix, uint64_t* out);
int mkp_histogram_from_values(const float* vals, uint64_t n, uint32_t level, uint32_t prefix, uint64_t* out);  /* host values, no device */
int mkp_histogram_locate(const uint64_t* hist0, float q, uint32_t bins[2], uint64_t ranks_in_bin[2], uint64_t* n);
int mkp_histogram_resolve(uint32_t prefix, const uint64_t* hist1, uint64_t rank_in_bin, float* value);
int mkp_percentile_from_histogram(uint64_t n, float q, float y_floor, float y_ceil, float* out);

/* ---- pileup-hemi: duplex (hemi-methylation) pattern counts.  Stands in for process_region_duplex_batch
 * (src/pileup/duplex.rs:209-339) over every interval inside a shard, with DuplexReadCache::get_duplex_mod_call
 * (src/read_cache.rs:422-462) and DuplexFeatureVector::decode (duplex.rs:124-205) on the device.
 * Rows = DuplexPatternCounts (duplex.rs:32-56) + the position's n_delete, SoA, in the order the reference's writer emits them
 * (position, primary base by letter, pattern — src/writers.rs:185-258).  A pattern element is MKP_HEMI_CANONICAL for '-'
 * (a canonical call) or the mod code (code_repr encoding above); DuplexModCodeRepr's order is the numeric order of that. */
#define MKP_HEMI_CANONICAL 0u
typedef struct {
  uint64_t n_rows;
  const uint32_t* pos;
  const uint8_t* primary_base;      /* 'A','C','G','T': the record's SEQ base at the position, reference orientation */
  const uint32_t* pattern_pos;      /* call on the positive strand at `pos` */
  const uint32_t* pattern_neg;      /* call on the negative strand at the partner position */
  const uint32_t* n_valid;          /* valid_coverage = count + n_other_pattern */
  const uint32_t* count;
  const uint32_t* n_canonical;
  const uint32_t* n_other_pattern;
  const uint32_t* n_delete;
  const uint32_t* n_fail;
  const uint32_t* n_diff;
  const uint32_t* n_nocall;
  uint64_t processed_records, skipped_records;
} mkp_hemi_rows;
/* Run the shard begun with mkp_shard_begin / mkp_shard_add_records as pileup-hemi.  The shard's focus bytes must be those of
 * FocusPositions::MotifCombineStrands for ONE palindromic motif (rule bit 0 + a combo with a positive motif id mark the positions
 * that get rows).  partner_offset = MotifInfo::negative_strand_position(p) - p (src/motif_bed.rs:124-140; 1 for CG,0).
 * interval_starts = ascending start positions of the reference's intervals inside [start,end) (ReferenceIntervalsFeeder,
 * src/interval_chunks.rs:497-652): the reference keeps one read cache per interval, which shows in the output only through
 * records whose tags fail to parse (one NoCall per such record and interval); NULL / 0 = the shard is one interval.
 * mkp_shard_rerun re-launches the hemi kernels afterwards (pass out = NULL there). */
int mkp_hemi_shard_run(mkp_ctx* ctx, int32_t partner_offset, const uint32_t* interval_starts, uint32_t n_intervals, mkp_hemi_rows* out);
/* `modkit pileup-hemi <in.bam> -o <out.bed> [flags]` (DuplexModBamPileup::run, src/pileup/subcommand.rs:1122-1514):
 * argv = the arguments after the subcommand name; without -o the rows go to stdout. */
int mkp_pileup_hemi_main(int argc, const char* const* argv, char* errbuf, size_t errbuf_len);
int mkp_pileup_hemi_run(mkp_ctx* ctx, int argc, const char* const* argv, mkp_run_report* report);

/* ---- `modkit sample-probs` (SampleModBaseProbs, src/commands.rs:549-887), the percentiles table: the reads the reference's schedule
 * samples are decoded on the device (the sampling kernels of the threshold estimate); per canonical base the requested percentiles of
 * their argmax probabilities come out of the HBM-resident sample exactly (Percentiles::new -> percentile_linear_interp,
 * src/thresholds.rs:17-38).  argv = the subcommand's sampling flags (-n -f --no-sampling --region -i --include-bed --only-mapped
 * --ignore --edge-filter --invert-edge-filter -t); values[b * n_percentiles + k] for bases A,C,G,T; has[b] = 0 when the sample holds
 * no call on base b; n_values[b] = sampled calls on base b.  A base with fewer than two values fails with MKP_E_THRESHOLD, as the
 * reference does.  (The histogram / plot outputs of the subcommand are outside this path.)
 * A BAM without an index file takes the reference's serial branch (src/reads_sampler/mod.rs:129-158), as mkp_summary and the estimate of
 * mkp_extract_calls_main do: no schedule, the file in file order under RecordSampler — the first -n records that yield values, or with
 * -f < 1 one `gen_bool` per record from rand's StdRng, which needs --seed (src/reads_sampler/record_sampler.rs:29-38, 80-86; without a
 * seed the reference draws from entropy: MKP_E_UNSUPPORTED); --region is then an error, as in the reference.  With an index, -f < 1 only
 * draws for the records without coordinates (--seed again). */
int mkp_sample_probs(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv, const float* percentiles, uint32_t n_percentiles,
                     float* values, uint8_t has[4], uint64_t n_values[4]);

/* ---- `modkit summary` (ModSummarize, src/commands.rs:888-1189 -> summarize_modbam / sampled_reads_to_summary, src/summarize.rs:59-262):
 * ModSummary as counts.  The sampled reads are decoded twice by the sampling kernels: once to estimate the pass thresholds (skipped with
 * --no-filtering / --filter-threshold), once to count every sampled call under its thresholded call — or, when that is Filtered, under
 * its argmax call.  argv = the subcommand's flags (-n -f --no-sampling --region -i --include-bed --only-mapped --ignore --edge-filter
 * --invert-edge-filter -p --no-filtering --filter-threshold --mod-thresholds -t).  Rows: for every canonical base with sampled calls
 * the canonical state (code_repr = MKP_HEMI_CANONICAL) then every observed mod code in code order; arrays owned by the ctx until its
 * next summary call.  (The table / TSV writers iterate std HashMaps and print through f32 Display: they stay in Rust.) */
typedef struct {
  uint64_t total_reads_used;
  uint64_t reads_with_mod_calls[4];     /* per canonical base A,C,G,T */
  float threshold[4]; uint8_t has_threshold[4];
  uint32_t n_rows;
  const uint8_t* base;                  /* 0..3 */
  const uint32_t* code_repr;
  const uint64_t* pass_count;           /* mod_call_counts */
  const uint64_t* fail_count;           /* filtered_mod_call_counts */
} mkp_summary_out;
int mkp_summary(mkp_ctx* ctx, const char* bam_path, int argc, const char* const* argv, mkp_summary_out* out);

/* ---- `modkit extract calls <in.bam> <out.tsv> [flags]` (EntryExtractCalls::run, src/extract/subcommand.rs:452-761): the per-read call table
 * (PositionModCalls::header / to_row, src/extract/writer.rs:12-132) — 21 tab-separated columns per call: read id, forward and reference
 * position, strands, soft clips, read length, call_prob / call_code (BaseModProbs::argmax_base_mod_call), base quality, reference and
 * query k-mers, canonical / modified primary base, fail (MultipleThresholdModCaller::call == Filtered), inferred, within_alignment, flag.
 * The calls (MM / ML decode, edge filter, --ignore collapse, argmax and thresholded call) are computed on the device; ids, positions,
 * qualities, k-mers and the text on the host.  argv = in.bam out.tsv + --ref fa, --allow-non-primary, --mapped-only, --pass-only,
 * --no-headers, --kmer-size k, --no-filtering | --filter-threshold .. | the sampling flags of the threshold estimate (-n -f -p -t
 * --sampling-interval-size), --mod-thresholds, --ignore, --edge-filter, --invert-edge-filter, --device N.  Records go out in FILE order
 * (the reference's serial path, which its golden tests pin; its indexed path emits interval batches in Rayon completion order).
 * Round 6: --include-bed (ReferencePositionFilter::keep, src/extract/util.rs:44-69: rows are asked of the BED with the reference strand
 * of the mod; rows without a reference position go), --region (src/extract/util.rs:126-160: steers the threshold estimate; with a BAI next
 * to the BAM and without --ignore-index the table holds the records overlapping the region — what the reference's interval fetches
 * return — otherwise every record of the file, as its serial scan does), --num-reads N with --ignore-index or an unindexed BAM (the first N
 * records that reach process_record, util.rs:519-575), --ignore-index.
 * --num-reads N on an indexed BAM follows the reference's sampling schedule (run_extract_reads, src/extract/util.rs:329-470;
 * SamplingSchedule::from_num_reads + get_record_sampler, src/reads_sampler/sampling_schedule.rs:171-273, 417-438): one sampler per interval
 * of the feeder (with --include-bed: of the BED-optimised reference records), then the records without coordinates; rows in interval order.
 * --ignore-implicit drops the inferred calls where the reference does: in its interval path (an index, no --ignore-index; util.rs:413-419) — its
 * serial scan takes the flag and never looks at it.  --exclude-bed drops the rows whose reference position and reference mod strand the BED
 * lists (ReferencePositionFilter::keep, util.rs:44-69).  --motif M off / --cpg (with --ref, --mask): the include filter becomes the motif hits
 * over the whole contigs, intersected with --include-bed (load_regions, util.rs:157-277).  --seed goes to the estimate.  --bgzf writes the table as
 * BGZF blocks (SAM spec 4.1) closed by the EOF block. */
int mkp_extract_calls_main(int argc, const char* const* argv, char* errbuf, size_t errbuf_len);

/* ---- `modkit stats <in.bed.gz> --regions <bed>` (EntryStats::run, src/stats/subcommand.rs:65-206; GenomeRegion::into_stats,
 * src/stats/mod.rs:53-101): per region and mod code the sums of N_mod and N_valid_cov over the bedMethyl rows whose start lies in
 * [start, end), whose strand overlaps the region's rule (StrandRule::overlaps, src/util.rs:310-318: either side '.', or equal) and whose
 * N_valid_cov >= min_coverage — reduced on the device from row columns that are in HBM (mkp_stats.hip), so that a pileup run can be
 * aggregated without its rows ever being read back, written as text, compressed and indexed.  The table lives in HBM from
 * mkp_stats_begin to mkp_stats_get and every add call adds into it: a region that straddles shard seams gets each row once.
 *   mkp_stats_begin         regions in the caller's order (tid < 0: a contig the rows cannot be on), start <= end (start == end: an empty
 *                           region, all zeros); codes = `--mod-codes` (only these are counted; duplicates collapse), n_codes = 0: every
 *                           code met.  At most 16 distinct codes per run, more is MKP_E_UNSUPPORTED (reported by mkp_stats_get at the
 *                           latest).  min_coverage = `--min-coverage` (the reference's default is 1).
 *   mkp_stats_add_resident  the rows the last mkp_shard_run / mkp_shard_rerun on this ctx left in HBM (the shard's contig and window);
 *                           MKP_E_INVALID with partition tags set (rows grouped by key are not in genome order) or after a hemi run.
 *   mkp_stats_add_rows      rows the caller holds (the bedMethyl-file form: fetch_region of src/tabix.rs:103-154 + BedMethylLine,
 *                           src/dmr/bedmethyl.rs:40-86), one contig per call, ascending pos (MKP_E_INVALID otherwise): pos, strand,
 *                           code_repr, n_valid and n_mod are read, uploaded, and go through the same kernels.
 *   mkp_stats_get           waits for the device and returns the table: columns = the given codes, sorted, or the codes that had a counted
 *                           row in some region (a counted row with N_mod == 0, or with N_valid_cov == 0 under min_coverage 0, still
 *                           makes the column; a code met only outside the regions does not), in ModCodeRepr order.  contig_has_rows[r]
 *                           = an add call brought at least one row (before any filter) on region r's contig: the reference drops the
 *                           other regions (HtsTabixHandler::has_contig, subcommand.rs:127-140).  Arrays owned by the ctx until its next
 *                           mkp_stats_begin.  percent_modified = (n_mod as f32 / n_valid as f32) * 100 (ModPositionInfo, util.rs:920-936)
 *                           is left to the table writer. */
typedef struct { int32_t tid; uint32_t start, end; uint8_t strand_rule; /* 1 '+', 2 '-', 3 both */ uint8_t pad[3]; } mkp_region;
typedef struct { uint32_t n_regions, n_codes; const uint32_t* code_repr;      /* sorted */
                 const uint64_t* n_mod; const uint64_t* n_valid;              /* [region * n_codes + code] */
                 const uint8_t* contig_has_rows;                              /* per region: 0 = the reference would drop it */ } mkp_stats_out;
int mkp_stats_begin(mkp_ctx* ctx, const mkp_region* regions, uint32_t n, const uint32_t* codes, uint32_t n_codes /*0 = all observed*/, uint64_t min_coverage);
int mkp_stats_add_resident(mkp_ctx* ctx);
int mkp_stats_add_rows(mkp_ctx* ctx, int32_t tid, const mkp_rows* rows);
int mkp_stats_get(mkp_ctx* ctx, mkp_stats_out* out);
/* Host-only halves of the same subcommand (no device needed).
 * mkp_host_parse_regions: the regions BED as EntryStats::run reads it (subcommand.rs:79-110; GenomeRegion::parse_unstranded_bed_line /
 *   parse_stranded_bed_line, src/util.rs:864-909): the first line that does not start with '#' picks the parser by its number of
 *   tab-separated fields (<= 4: chrom start end [name], both strands; otherwise chrom start end name score strand with score a float or
 *   '.'), then EVERY line goes through it — a '#' line, an empty file or any other unparsable line fails (MKP_E_INVALID), as does
 *   start > end.  contig_names give the tids (a chrom that is not among them gets tid -1).  A name holding a quote, or a coordinate
 *   beyond 2^32 - 1, is MKP_E_UNSUPPORTED.  The set is freed with mkp_region_set_free.
 * mkp_host_stats_table: the table EntryStats::run writes (MethylationStats::header / into_row, src/stats/mod.rs:24-51, through the csv
 *   writer with a tab delimiter): `chrom start end name strand` then count_<c> count_valid_<c> percent_<c> per code, regions in file order
 *   without those whose contig_has_rows is 0, an absent name as '.', the percentage through f32 Display. */
typedef struct mkp_region_set mkp_region_set;
int mkp_host_parse_regions(const char* bed_path, const char* const* contig_names, uint32_t n_contigs, mkp_region_set** out, char* errbuf, size_t errbuf_len);
uint32_t mkp_region_set_size(const mkp_region_set* set);
const mkp_region* mkp_region_set_regions(const mkp_region_set* set);
const char* mkp_region_set_chrom(const mkp_region_set* set, uint32_t i);
const char* mkp_region_set_name(const mkp_region_set* set, uint32_t i);   /* "." when the line has none */
void mkp_region_set_free(mkp_region_set* set);
int mkp_host_stats_table(const mkp_region_set* set, const mkp_stats_out* counts, int with_header, const char* out_path);

/* ---- `modkit localize <in.bed.gz> --regions <bed> --genome-sizes <tsv>` (EntryLocalize::run, src/localise/subcommand.rs:211-305;
 * GenomeRegion::into_localized_mod_counts and LocalizedModCounts, src/localise/util.rs:25-82, 189-227): per mod code and offset from a
 * feature's anchor the sums of N_mod and N_valid_cov over all features — an LDS-privatised histogram over row columns that are in HBM
 * (mkp_localize.hip).  The table lives in HBM from mkp_localize_begin to mkp_localize_get and every add call adds into it: a window
 * that straddles shard seams gets each row once.  A stats run and a localize run may be open on one ctx at the same time.
 *   mkp_localize_begin         regions as parsed (start > end is allowed, as in the reference); contig_len_by_tid = the genome-sizes table
 *                              (a region with tid < 0 or >= n_contigs is dropped: load_focus_regions, subcommand.rs:163-187).  The window
 *                              arithmetic is done here, in 64 bits: mp = (start + end) / 2, ws = mp - (window + 1) or 0 when that
 *                              underflows, we = min(mp + window, contig length), anchor = (ws + we) / 2 (GenomeRegion::midpoint of the
 *                              EXPANDED region, src/util.rs:860-862: mp - 1 for an unclipped window); we <= ws is an empty window.  Every
 *                              offset of a non-empty window lies in [-window, window] (checked per region).  stranded = `--stranded`
 *                              (0 none, 1 same, 2 opposite), stranded_features = `--stranded-features` (0 = each region's own strand,
 *                              1 '+', 2 '-', 3 '.').  window > 100 000 and a contig longer than 2^32 - 1 are MKP_E_UNSUPPORTED; no
 *                              region on a listed contig is MKP_E_INVALID ("failed to find any valid regions").  `--min-coverage` is
 *                              not offered: the reference parses and logs it and filters nothing by it (subcommand.rs:215-216).
 *   mkp_localize_add_resident  the rows the last mkp_shard_run / mkp_shard_rerun on this ctx left in HBM; refusals as mkp_stats_add_resident.
 *   mkp_localize_add_rows      rows the caller holds, one contig per call, ascending pos; as mkp_stats_add_rows (fetch_region,
 *                              src/tabix.rs:141-154).
 *   mkp_localize_get           waits for the device and returns the table.  A row is counted when pos is in [ws, we), its strand
 *                              overlaps the fetch rule (stranded_features, else the region's strand: BedMethylLine::overlaps,
 *                              src/tabix.rs:24-31, StrandRule::overlaps, src/util.rs:310-318) and, under `same`,
 *                              region.strand.overlaps(row.strand) holds — under `opposite`, does not hold (a '.' region keeps nothing,
 *                              a '.' row is always dropped).  offset = anchor - pos: upstream on the reference is positive, whatever
 *                              the strand.  Codes = those with a counted row, in ModCodeRepr order; arrays [code * (2 window + 1) +
 *                              offset + window]; n_rows = counted rows of the cell (the reference writes a line for every cell that
 *                              had one, also with N_valid_cov 0).  A region whose contig no add call brought a row on is dropped; when
 *                              none is left, MKP_E_INVALID, as the reference fails.  A seventeenth code inside a window is
 *                              MKP_E_UNSUPPORTED.  Arrays owned by the ctx until its next mkp_localize_begin.
 *   mkp_localize_tile_offsets  the offsets a workgroup of the reduce kernel owns (for tests that put a tile edge inside a table). */
typedef struct { uint32_t n_codes, window; const uint32_t* code_repr;                      /* sorted */
                 const uint64_t* n_mod; const uint64_t* n_valid; const uint64_t* n_rows;   /* [code * (2 window + 1) + offset + window] */
               } mkp_localize_out;
int mkp_localize_begin(mkp_ctx* ctx, const mkp_region* regions, uint32_t n, const uint64_t* contig_len_by_tid, uint32_t n_contigs, uint32_t window,
    int stranded /*0 none, 1 same, 2 opposite*/, int stranded_features /*0 the region's own, 1 '+', 2 '-', 3 '.'*/);
int mkp_localize_add_resident(mkp_ctx* ctx);
int mkp_localize_add_rows(mkp_ctx* ctx, int32_t tid, const mkp_rows* rows);
int mkp_localize_get(mkp_ctx* ctx, mkp_localize_out* out);
uint32_t mkp_localize_tile_offsets(void);
/* Host-only halves (no device needed).
 * mkp_host_parse_localize_regions: the regions BED as load_focus_regions reads it (subcommand.rs:105-162): the first line that does not
 *   start with '#' picks the parser by its number of WHITESPACE-separated fields (<= 4: bed3/4, both strands; otherwise chrom start end name
 *   score strand), then every line goes through it; a line that fails is skipped and counted in *n_skipped, the load fails (MKP_E_INVALID)
 *   only when no line parsed.  No start <= end check.  A coordinate beyond 2^32 - 1 is MKP_E_UNSUPPORTED.
 * mkp_host_parse_genome_sizes: `chrom<whitespace>length` per line (read_sequence_lengths_file, src/util.rs:969-990); any line that does
 *   not parse fails (MKP_E_INVALID); of two lines for one contig the later length holds, at the earlier one's place.
 * mkp_host_localize_table: the table LocalizedModCounts::get_table gives (util.rs:48-82) through the tab-delimited csv writer:
 *   `mod_code offset n_valid n_mod percent_modified`, a line per (code, offset) with n_rows > 0, codes in ModCodeRepr order, offsets
 *   ascending, percent_modified = (n_mod as f32 / n_valid as f32) * 100 or 0 (ModPositionInfo, src/util.rs:920-936) through f32 Display. */
int mkp_host_parse_localize_regions(const char* bed_path, const char* const* contig_names, uint32_t n_contigs, mkp_region_set** out,
    uint32_t* n_skipped, char* errbuf, size_t errbuf_len);
typedef struct mkp_genome_sizes mkp_genome_sizes;
int mkp_host_parse_genome_sizes(const char* path, mkp_genome_sizes** out, char* errbuf, size_t errbuf_len);
uint32_t mkp_genome_sizes_size(const mkp_genome_sizes* sizes);
const char* mkp_genome_sizes_name(const mkp_genome_sizes* sizes, uint32_t i);
uint64_t mkp_genome_sizes_length(const mkp_genome_sizes* sizes, uint32_t i);
void mkp_genome_sizes_free(mkp_genome_sizes* sizes);
int mkp_host_localize_table(const mkp_localize_out* counts, const char* out_path);

/* ---- `modkit bedmethyl merge` (merge_data, src/bedmethyl_util/subcommands.rs:136-195) on the device (mkp_merge.hip): an outer join of
 * bedMethyl row sets on (start, mod code, strand) that sums valid_coverage and the seven other counts.  One merged row table per contig
 * lives in HBM from mkp_merge_begin on; every add is one two-way merge of the contig's table with the rows added.
 *   mkp_merge_begin         contig_len_by_tid = the genome-sizes table (or the BAM header's lengths); frees the tables of the session
 *                           before.  A contig longer than 2^32 - 1 is MKP_E_UNSUPPORTED.
 *   mkp_merge_add_rows      rows of ONE contig, all eleven columns (pos, strand, code_repr, n_valid .. n_nocall), ascending pos
 *                           (MKP_E_INVALID otherwise), in any order inside a position; motif_idx is not read.  Rows that share a key are
 *                           summed even inside one call, as the reference puts every line of every input into one map (two motifs at one
 *                           position collapse).  Rows at pos >= the contig's length, or on a tid the sizes do not list, are dropped and
 *                           counted (the reference's feeder walks [0, length) of the listed contigs).
 *   mkp_merge_add_resident  the rows the last mkp_shard_run / mkp_shard_rerun on this ctx left in HBM (their motif is dropped); refusals as
 *                           mkp_stats_add_resident.
 *   mkp_merge_get           the merged rows of one contig, ordered by start, then strand ('+' < '-' < '.'), then code (ModCodeRepr's derived Ord,
 *                           which the reference's sort calls: letters by code point, then ChEBI numbers by number): all columns of mkp_rows, motif_idx = -1, no
 *                           partition keys.  A contig without rows gives n_rows = 0.  *n_dropped (may be NULL) = the rows dropped since
 *                           mkp_merge_begin.  A summed count beyond 2^32 - 1 is MKP_E_UNSUPPORTED (rows carry 32-bit counts, the reference
 *                           sums in 64 bits; a wrapped value is never returned), as is a position that holds more rows than a tile of
 *                           the merge kernel has room for (over a thousand; reported by the add that meets it).  Arrays owned by the ctx
 *                           until its next mkp_merge_begin / mkp_merge_get of the same contig.
 *   mkp_merge_tile_rows     the rows between two tile cuts of the merge kernel (for tests that put a run of equal keys on a tile edge).
 * The written line follows to_line (src/tabix.rs:33-74): the bare code as the name, score = column 10 = the summed valid_coverage,
 * percent = (n_mod as f32 / n_valid as f32) * 100 with {:.2}, `NaN` when n_valid is 0.
 * Input files are plain text or bgzip (BGZF) compressed, as the reference takes them (tabs and / or blanks; '#' lines skipped; the .tbi is
 * neither needed nor read).  A line that does not parse is MKP_E_IO with the line named (the reference drops its 100 kb chunk silently); a
 * truncated, damaged or CRC-failing BGZF block is MKP_E_IO with the block named; a gzip stream without BGZF blocks is MKP_E_UNSUPPORTED.
 *   mkp_merge_add_file      a whole bedMethyl file through the device reader (mkp_bedmethyl.hip): compressed blocks (or the plain bytes) go
 *                           up, are inflated, CRC-checked, cut into lines and parsed in HBM, and every run of lines on one contig is joined
 *                           where it lies; neither text nor rows visit the host.  contig_names[tid] = the names of the sizes table given to
 *                           mkp_merge_begin: rows of a chrom not among them, or at pos >= the contig's length, are dropped and counted.
 *                           pos must not descend inside a run of lines on one contig (MKP_E_INVALID, the line named).  The file is read in
 *                           pieces of at most MKP_BEDMETHYL_PIECE_KB KiB of text (default 131072, least 64); a line that does not fit one is
 *                           MKP_E_UNSUPPORTED (the host reader has no such limit).  *n_rows (may be NULL) = the file's rows.
 *   mkp_bedmethyl_read_device  the same reader, the rows copied back into a mkp_bedmethyl_file (a run cut by a piece seam comes back as one).
 *   mkp_bedmethyl_chunk_bytes  the bytes of text a workgroup of the reader's line kernels takes (for tests that put line ends on its edges).
 * Host-only half: mkp_host_read_bedmethyl reads the same files on the CPU (BGZF through the host's own inflate, CRC checked) into runs of
 * lines on one contig.  mkp_bedmethyl_file_rows fills the eleven columns of run `run` (arrays owned by the file object).
 * mkp_bedmethyl_merge_main = `mkpileup bedmethyl merge a.bed b.bed [..] -g sizes.tsv -o out.bed [--force] [--bgzf] [--device N] [--stats]`:
 * contigs come out in the order of the sizes file, those without a row are not written; *n_written / *n_dropped may be NULL. */
int mkp_merge_begin(mkp_ctx* ctx, const uint64_t* contig_len_by_tid, uint32_t n_contigs);
int mkp_merge_add_rows(mkp_ctx* ctx, int32_t tid, const mkp_rows* rows);
int mkp_merge_add_resident(mkp_ctx* ctx);
int mkp_merge_get(mkp_ctx* ctx, int32_t tid, mkp_rows* out, uint64_t* n_dropped);
uint32_t mkp_merge_tile_rows(void);
typedef struct mkp_bedmethyl_file mkp_bedmethyl_file;
int mkp_host_read_bedmethyl(const char* path, mkp_bedmethyl_file** out, char* errbuf, size_t errbuf_len);
uint32_t mkp_bedmethyl_file_runs(const mkp_bedmethyl_file* file);
const char* mkp_bedmethyl_file_chrom(const mkp_bedmethyl_file* file, uint32_t run);
int mkp_bedmethyl_file_rows(const mkp_bedmethyl_file* file, uint32_t run, mkp_rows* out);
void mkp_bedmethyl_file_free(mkp_bedmethyl_file* file);
int mkp_merge_add_file(mkp_ctx* ctx, const char* path, const char* const* contig_names, uint32_t n_names, uint64_t* n_rows);
int mkp_bedmethyl_read_device(mkp_ctx* ctx, const char* path, mkp_bedmethyl_file** out);
uint32_t mkp_bedmethyl_chunk_bytes(void);
int mkp_bedmethyl_merge_main(int argc, const char* const* argv, uint64_t* n_written, uint64_t* n_dropped, char* errbuf, size_t errbuf_len);

/* ---- `modkit dmr pair -a a.bed.gz -b b.bed.gz -r regions.bed --ref ref.fa --base C` (PairwiseDmr::run with -r, src/dmr/subcommands.rs;
 * pairwise.rs, bedmethyl.rs:172-267, llr_model.rs, genome_positions.rs:91-127): every region scored for differential methylation between
 * two bedMethyl tables.  The rows are filtered, grouped by position, checked and summed on the device from row columns that are in HBM
 * (mkp_dmr.hip); the table of sums lives there from mkp_dmr_begin to mkp_dmr_get and every add call adds into it.  Only the region form
 * of one `a` against one `b`: single-site mode is mkp_dmr_sites_* below, --segment and `dmr multi` are not offered.
 *   mkp_dmr_begin           regions as mkp_stats_begin takes them; bases = the `--base` letters (each of ACGT, at least one); codes /
 *                           code_bases = the code -> base table, n_lookup entries (mkp_dmr_default_lookup gives MOD_CODE_TO_DNA_BASE; a
 *                           later entry for a code replaces an earlier one, as `--assign-code` does; at most 64 distinct codes);
 *                           min_valid_coverage = `--min-valid-coverage`; respect_mask = `--mask` (a lower-case reference byte is no base).
 *   mkp_dmr_set_reference   the reference bytes [offset, offset + len) of contig tid, uploaded once; positions outside have no base.  The
 *                           command uploads the span from the contig's lowest region start to its highest region end.  A contig without
 *                           this call is one the FASTA does not hold: its regions are not written.  Before the contig's rows.
 *   mkp_dmr_add_rows        rows of sample 0 (a) or 1 (b) the caller holds, one contig per call, ascending pos, as mkp_stats_add_rows; pos,
 *                           strand, code_repr, n_valid, n_mod and n_canonical are read.  A row takes part when N_valid_cov >=
 *                           min_valid_coverage, its code is in the table, the reference base at pos is the code's base ('+' and '.' rows)
 *                           or its complement ('-' rows), and get_positions lists that base on that strand for the region's rule (a base
 *                           of the positive set counts as positive where the rule covers '+').  The rows of a position that take part
 *                           must agree on N_valid_cov and N_canonical, and N_canonical + sum N_mod must equal N_valid_cov; otherwise the
 *                           (sample, region) is bad.  Pieces of a contig come in ascending order; a position may be cut by a seam (its
 *                           rows are held back until the next piece, another contig or mkp_dmr_get), with at most 64 rows a position.
 *   mkp_dmr_add_file        a whole bedMethyl file, plain or bgzip, through the device reader (mkp_merge_add_file): the rows never reach
 *                           the host; contig_names[tid]; rows of another chrom are not counted.  *n_rows (may be NULL) = the file's rows.
 *   mkp_dmr_add_resident    the rows the last mkp_shard_run left in HBM, as sample `sample`; refusals as mkp_stats_add_resident.
 *   mkp_dmr_get             waits for the device and returns, per sample (a, b) and region: n_mod per code column (columns = the codes a
 *                           participating row carried in some region, ModCodeRepr order; at most 16 per run, more is MKP_E_UNSUPPORTED),
 *                           has_code (the sample's key set holds the code: a participating row carried it, N_mod == 0 too), total (the
 *                           N_valid_cov of every position once), n_rows (participating rows), bad, contig_has_rows (an add call brought
 *                           a row on the region's contig); has_reference; score = llk_ratio, computed on the host in f64; state = why a
 *                           region is not written (MKP_DMR_*; a region with no participating row is written: `.` counts, score 0).
 *                           Arrays owned by the ctx until its next mkp_dmr_begin.
 * Host-only: mkp_host_parse_dmr_regions = parse_roi_bed (src/dmr/util.rs:389-428): as mkp_host_parse_regions, but the '#' lines in front
 *   are skipped and a quote in a name is kept.  mkp_host_dmr_table writes ModificationCounts::header (names a and b) / to_row of the regions
 *   whose state is MKP_DMR_WRITTEN, in file order: a line without a name gets chrom:start-end, the score goes through f64 Display (shortest
 *   digits that round-trip, never an exponent), percentages `{:.2}` of (n as f32 / total as f32) * 100, pct_modified through f32 Display
 *   (`NaN` at total 0).  score and state are read as given: a caller that fills the counts itself calls mkp_host_dmr_judge first.
 * mkp_dmr_pair_main = `mkpileup dmr pair -a a.bed[.gz] -b b.bed[.gz] -r regions.bed --ref ref.fa --base C [--base A ..] [-o out.bed] [-f]
 *   [--header] [--min-valid-coverage N] [--assign-code x:C] [--mask] [--missing quiet|warn|fail] [--device N] [--stats]`; *n_written (may be
 *   NULL) = the regions written.  A region that ends beyond its contig in the FASTA is MKP_E_INVALID (the reference panics). */
enum { MKP_DMR_WRITTEN = 0, MKP_DMR_NO_CONTIG = 1 /* absent from a table */, MKP_DMR_NO_REFERENCE = 2, MKP_DMR_BAD = 3 /* an inconsistent
       position in a sample */, MKP_DMR_MODEL = 4 /* llk_ratio fails: one code against a different code */ };
typedef struct { uint32_t n_regions, n_codes; const uint32_t* code_repr;       /* sorted */
                 const uint64_t* n_mod[2]; const uint8_t* has_code[2];         /* per sample: [region * n_codes + code] */
                 const uint64_t* total[2]; const uint64_t* n_rows[2];          /* per sample: [region] */
                 const uint8_t* bad[2]; const uint8_t* contig_has_rows[2];
                 const uint8_t* has_reference; const double* score; const uint8_t* state; } mkp_dmr_out;
uint32_t mkp_dmr_default_lookup(uint32_t* codes, uint8_t* code_bases, uint32_t cap);   /* returns the entries (17) */
int mkp_dmr_begin(mkp_ctx* ctx, const mkp_region* regions, uint32_t n, const char* bases, uint32_t n_bases, const uint32_t* codes,
                  const uint8_t* code_bases, uint32_t n_lookup, uint64_t min_valid_coverage, int respect_mask);
int mkp_dmr_set_reference(mkp_ctx* ctx, int32_t tid, const uint8_t* bytes, uint32_t offset, uint32_t len);
int mkp_dmr_add_rows(mkp_ctx* ctx, int sample, int32_t tid, const mkp_rows* rows);
int mkp_dmr_add_file(mkp_ctx* ctx, int sample, const char* path, const char* const* contig_names, uint32_t n_names, uint64_t* n_rows);
int mkp_dmr_add_resident(mkp_ctx* ctx, int sample);
int mkp_dmr_get(mkp_ctx* ctx, mkp_dmr_out* out);
int mkp_host_parse_dmr_regions(const char* bed_path, const char* const* contig_names, uint32_t n_contigs, mkp_region_set** out, char* errbuf,
                               size_t errbuf_len);
int mkp_host_dmr_judge(const mkp_dmr_out* counts, double* score, uint8_t* state);
int mkp_host_dmr_table(const mkp_region_set* set, const mkp_dmr_out* counts, int with_header, const char* out_path);
int mkp_dmr_pair_main(int argc, const char* const* argv, uint64_t* n_written, char* errbuf, size_t errbuf_len);

/* ---- `modkit dmr pair -a a.bed.gz -b b.bed.gz --ref ref.fa --base C` without -r (SingleSiteDmrAnalysis::run, src/dmr/single_site.rs;
 * beta_diff.rs, llr_model.rs): the two tables compared position by position; every site both hold gets the likelihood-ratio score and the
 * MAP-based p-value with its effect size, in f64 on the device (mkp_dmr_sites.hip, one lane a site).  One `a` against one `b`: replicates
 * are mkp_dmr_reps_* below; --segment is not offered.  Both tables' row columns stay in HBM per contig from the add calls to mkp_dmr_sites_get (24 B a row); a
 * pair of tables beyond the budget of 3/4 of the device's memory is MKP_E_UNSUPPORTED.
 *   mkp_dmr_sites_begin          cfg: contig_names[tid] (contigs are walked in byte order of their names); bases / codes / code_bases /
 *                                min_valid_coverage / respect_mask as mkp_dmr_begin; prior Beta(prior_alpha, prior_beta) (alpha + beta < 1
 *                                is MKP_E_INVALID); delta = the region of practical equivalence; have_max_coverages != 0: max_coverages =
 *                                `--max-coverages`, otherwise they are estimated from the first n_sample_records participating rows
 *                                (calculate_max_coverages); either way capped at 300; interval_size and batch_size shape the reference's
 *                                batches (below).
 *   mkp_dmr_sites_set_reference  the WHOLE sequence of contig tid, any time before mkp_dmr_sites_get.  A contig without it is one the FASTA lacks.
 *   mkp_dmr_sites_add_rows       rows of sample 0 (a) or 1 (b), one contig per call, ascending pos, pieces of a contig in ascending order (a
 *                                seam may cut a position: the contig's pieces are joined in HBM); the six columns mkp_dmr_add_rows reads.
 *   mkp_dmr_sites_add_file       a whole bedMethyl file, plain or bgzip, through the device reader, as mkp_dmr_add_file.
 *   mkp_dmr_sites_get            runs the stages and returns the written sites by contig (sorted by name), then position.  The contigs are
 *                                those with a reference and rows in both samples; none is MKP_E_INVALID ("need at least 1 contig").  A row
 *                                takes part as in mkp_dmr_add_rows under a '.' rule.  The reference's walk cuts every contig into windows
 *                                of interval_size bp; a batch collects windows until it holds interval_size listed positions (it may run
 *                                on into the next contig), batch_size batches are a super-batch.  A position whose participating rows
 *                                fail aggregate_counts drops its whole batch for both samples (n_batches_dropped).  A site whose score or
 *                                p-value fails in the reference is not written (n_model_failures).  n_mod[s][site * n_codes + k],
 *                                has_code[s][site] = mask of the code columns in the sample's key set; n_sampled = the coverages the
 *                                estimate drew per sample (0 with given max coverages).  Arrays owned by the ctx until its next
 *                                mkp_dmr_sites_begin; the session stays open and may be run again.
 * Host-only: mkp_host_dmr_site_score = the arithmetic of one site as the kernel does it (mkp_dmr_site_math.hpp): values[5] = score,
 *   ln_effect, ln_null, map_pvalue, effect_size (NaN where the reference does not compute one); *failed = the reference fails on the site.
 *   mkp_host_dmr_sites_batches = the batch planner alone: contig_len[c] and, one contig behind the other, the listed positions per window
 *   (max(1, ceil(len / interval_size)) windows a contig); entries (at most one per window; cap of them are written) say where a batch
 *   begins inside a contig; returns their number (or a negative status), *n_batches the batches.  mkp_host_dmr_sites_gauss_legendre = the 16 nodes and weights.
 *   mkp_host_dmr_sites_table writes SingleSiteDmrScore::header(false, false) / to_row_pair: 16 tab-separated columns, the three f64 values
 *   through f64 Display.
 * mkp_dmr_sites_main = `mkpileup dmr sites -a a.bed[.gz] -b b.bed[.gz] --ref ref.fa --base C [--base A ..] [-o out.bed] [-f] [--header]
 *   [--min-valid-coverage N] [--assign-code x:C] [--mask] [--prior ALPHA BETA] [--delta D] [--max-coverages A B] [-N/--n-sample-records N]
 *   [--cap-coverages] [-i/--interval-size BP] [--batch-size N | -t/--threads T] [--device N] [--stats]`; *n_written (may be NULL) = the sites
 *   written.  -r is MKP_E_INVALID (that is `dmr pair`), --segment and more than one -a / -b (replicates: that is `dmr replicates`) are
 *   MKP_E_UNSUPPORTED. */
typedef struct { const char* const* contig_names; uint32_t n_contigs; const char* bases; uint32_t n_bases; const uint32_t* codes;
                 const uint8_t* code_bases; uint32_t n_lookup; uint32_t respect_mask; uint64_t min_valid_coverage; double prior_alpha, prior_beta,
                 delta; uint32_t have_max_coverages; uint32_t max_coverages[2]; uint32_t reserved; uint64_t n_sample_records, interval_size,
                 batch_size; } mkp_dmr_sites_config;
typedef struct { uint64_t n_sites; uint32_t n_codes, reserved; const uint32_t* code_repr;   /* sorted */
                 const int32_t* tid; const uint32_t* pos; const uint8_t* strand;             /* per site; strand '+' or '-' */
                 const uint32_t* total[2]; const uint32_t* n_mod[2]; const uint32_t* has_code[2];
                 const double* score; const double* map_pvalue; const double* effect_size;
                 uint32_t max_coverages[2]; uint64_t n_sampled[2]; uint64_t n_batches, n_batches_dropped, n_model_failures; } mkp_dmr_sites_out;
typedef struct { uint32_t contig, reserved; uint64_t start, batch; } mkp_dmr_sites_batch;
int mkp_dmr_sites_begin(mkp_ctx* ctx, const mkp_dmr_sites_config* cfg);
int mkp_dmr_sites_set_reference(mkp_ctx* ctx, int32_t tid, const uint8_t* bytes, uint64_t len);
int mkp_dmr_sites_add_rows(mkp_ctx* ctx, int sample, int32_t tid, const mkp_rows* rows);
int mkp_dmr_sites_add_file(mkp_ctx* ctx, int sample, const char* path, uint64_t* n_rows);
int mkp_dmr_sites_get(mkp_ctx* ctx, mkp_dmr_sites_out* out);
int mkp_host_dmr_site_score(const uint64_t* a_mod, uint32_t a_has, uint64_t a_total, const uint64_t* b_mod, uint32_t b_has, uint64_t b_total,
                            uint32_t n_codes, double prior_alpha, double prior_beta, double delta, const uint32_t max_coverages[2], double values[5],
                            int* failed);
int mkp_host_dmr_sites_batches(const uint64_t* contig_len, const uint32_t* window_counts, uint32_t n_contigs, uint64_t interval_size,
                               mkp_dmr_sites_batch* entries, uint64_t cap, uint64_t* n_batches);
int mkp_host_dmr_sites_gauss_legendre(double nodes[16], double weights[16]);
int mkp_host_dmr_sites_table(const mkp_dmr_sites_out* sites, const char* const* contig_names, uint32_t n_contigs, int with_header, const char* out_path);
int mkp_dmr_sites_main(int argc, const char* const* argv, uint64_t* n_written, char* errbuf, size_t errbuf_len);

/* ---- `modkit dmr pair -a a1.bed.gz -a a2.bed.gz .. -b b1.bed.gz -b b2.bed.gz .. --ref ref.fa --base C` without -r: replicates
 * (SingleSiteDmrScore::new_multi, collapse_counts, to_row, src/dmr/single_site.rs; SingleSiteSampleIndex, src/dmr/tabix.rs).  n_a >= 1 and
 * n_b >= 1 tables, at most 16 a side (more is MKP_E_UNSUPPORTED); multiple = n_a > 1 || n_b > 1, matched = n_a == n_b && n_a > 1.  Everything
 * mkp_dmr_sites_* says about rows, groups, batches, the contig walk and the two counters holds per sample; beyond it (mkp_dmr_reps.hip):
 *   - the contigs are those with a reference, rows in at least one `a` table and rows in at least one `b` table; a position whose group fails in
 *     ANY sample of EITHER side drops its batch for every sample;
 *   - a site is a position at least one `a` and one `b` sample hold; its present samples are listed in ascending command-line index (the
 *     reference takes the iteration order of an FxHashMap: a deliberate, deterministic departure);
 *   - total / n_mod / has_code, score, map_pvalue and effect_size come from the counts summed over the present samples (collapse_counts(_,
 *     false)); balanced_map_pvalue / balanced_effect_size from the coverage-balanced counts (collapse_counts(_, true), f32 arithmetic,
 *     mkp_dmr_reps_math.hpp); pct_samples[side][site] = floor(present / n * 100) in f32;
 *   - with matched sides and as many present `a` as `b` samples, n_rep[site] = that number and rep_pvalue / rep_effect[site * n_a + i] = the
 *     i-th present `a` sample against the i-th present `b` sample (pairing by rank); otherwise n_rep[site] = 0.  rep_pvalue and rep_effect
 *     are NULL unless matched;
 *   - a site any of whose evaluations fails (each replicate pair, the balanced p-value and likelihood ratio, the collapsed p-value and
 *     likelihood ratio) is not written and counted once in n_model_failures; where a sample's balanced counts sum beyond its balanced total
 *     the reference aborts (try_new(..).unwrap()): here that is a model failure as well;
 *   - the max coverages, given or estimated, are multiplied by the side's number of tables unless cap_coverages != 0 (`--cap-coverages`), then
 *     capped at 300 (PMapEstimator::new): sites.max_coverages reports these values;
 *   - estimated max coverages pool the coverages of the participating rows of all `a` samples, and of all `b` samples; sampling stops
 *     behind the super-batch at which both pools hold n_sample_records values;
 *   - a summed coverage beyond 2^32 - 1 is MKP_E_UNSUPPORTED.
 * mkp_dmr_reps_add_rows / _add_file take the side (0 = a, 1 = b) and the replicate (the table's index among the side's -a / -b); tables may
 * be added in any order, a contig's pieces of one table in ascending order.  All tables' row columns stay in HBM (24 B a row, 3/4 of the
 * device's memory at most).  With n_a == n_b == 1 the sites and the text are what mkp_dmr_sites_* give.
 * Host-only: mkp_host_dmr_reps_balance = collapse_counts(_, true) of one side of one site: n_samples present samples with
 *   n_mod[s * n_codes + k], has_code[s], total[s]; out_mod[n_codes], *out_has, *out_total; *failed = a sample's balanced counts exceed its
 *   balanced total.  mkp_host_dmr_reps_pct = the share of samples.  mkp_host_dmr_reps_table writes SingleSiteDmrScore::header(multiple,
 *   matched) / to_row: the 16 columns of mkp_host_dmr_sites_table, with `multiple` balanced_map_pvalue, balanced_effect_size, pct_a_samples,
 *   pct_b_samples, with `matched` replicate_map_pvalues and replicate_effect_sizes (comma-joined f64 Display, `-` where n_rep is 0).
 * mkp_dmr_reps_main = `mkpileup dmr replicates -a a1.bed[.gz] [-a a2.bed[.gz] ..] -b b1.bed[.gz] [-b ..] --ref ref.fa --base C` and every
 *   other flag of mkp_dmr_sites_main; -r is MKP_E_INVALID, --segment and more than 16 tables a side MKP_E_UNSUPPORTED. */
#define MKP_DMR_REPS_MAX_SIDE 16u
typedef struct { mkp_dmr_sites_out sites;   /* the 16 columns' values; total / n_mod / has_code = the collapsed counts */
                 uint32_t n_a, n_b;
                 const double* balanced_map_pvalue; const double* balanced_effect_size;
                 const uint32_t* pct_samples[2];
                 const uint32_t* n_rep; const double* rep_pvalue; const double* rep_effect; } mkp_dmr_reps_out;
int mkp_dmr_reps_begin(mkp_ctx* ctx, const mkp_dmr_sites_config* cfg, uint32_t n_a, uint32_t n_b, int cap_coverages);
int mkp_dmr_reps_set_reference(mkp_ctx* ctx, int32_t tid, const uint8_t* bytes, uint64_t len);
int mkp_dmr_reps_add_rows(mkp_ctx* ctx, int side, int replicate, int32_t tid, const mkp_rows* rows);
int mkp_dmr_reps_add_file(mkp_ctx* ctx, int side, int replicate, const char* path, uint64_t* n_rows);
int mkp_dmr_reps_get(mkp_ctx* ctx, mkp_dmr_reps_out* out);
int mkp_host_dmr_reps_balance(const uint64_t* n_mod, const uint32_t* has_code, const uint64_t* total, uint32_t n_samples, uint32_t n_codes,
                              uint64_t* out_mod, uint32_t* out_has, uint64_t* out_total, int* failed);
uint32_t mkp_host_dmr_reps_pct(uint32_t n_present, uint32_t n_samples);
int mkp_host_dmr_reps_table(const mkp_dmr_reps_out* sites, const char* const* contig_names, uint32_t n_contigs, int with_header, const char* out_path);
int mkp_dmr_reps_main(int argc, const char* const* argv, uint64_t* n_written, char* errbuf, size_t errbuf_len);

/* ---- BGZF inflate on the device as a call of its own.  On the pileup path the same kernels run inside the device ingest
 * (`mkp_pileup_main` on an indexed BAM: compressed blocks up, inflate + CRC-32 + record cut + MM/ML tokeniser + packing in HBM, a digest
 * back — DESIGN.md §3.6); this entry point exists so that the decoders are tested and measured alone.  Stands in for what htslib does
 * under rust-htslib's IndexedReader (src/pileup/mod.rs:732-743): BGZF blocks (SAM spec 4.1) of raw DEFLATE (RFC 1951) — neither htslib
 * nor zlib is part of the reference checkout, the decoders follow the RFC.  bgzf = n_bytes of whole BGZF blocks in host memory (a file
 * image).  One wave (small launches) or one thread (large ones) decodes a block; every block's CRC32 and ISIZE are checked before the
 * call returns.  *out = the inflated bytes, owned by the ctx until its next inflate call; *kernel_ms (may be NULL) = device time of the
 * decode kernel. */
int mkp_bgzf_inflate(mkp_ctx* ctx, const uint8_t* bgzf, uint64_t n_bytes, const uint8_t** out, uint64_t* out_len, double* kernel_ms);

/* ---- host-side pieces exposed for tests (no device needed):
 * mkp_host_mm_ranks: the packer's MM tokeniser (MmTagInfo::parse, src/mod_bam.rs:909-1000) on one MM string: for every tag its
 *   header (fundamental base A,C,G,T,N = 0..4; strand; mode 0 '?', 1 '.', 2 none; codes as code_repr) and its delta list turned into
 *   the cumulative occurrence ranks sum(d+1)-1 the device consumes (DeltaListConverter::to_positions_specific, 697-733, is rank ->
 *   position).  Returns the number of tags, or a negative status (MKP_E_INVALID = the reference would reject the tag).
 * mkp_host_map_order: iteration order of a small FxHashMap<ModCodeRepr, _> filled in the given insertion order (rustc-hash 1.1 +
 *   hashbrown), which decides probability ties in MultipleThresholdModCaller::call (src/threshold_mod_caller.rs:28-63). */
typedef struct { uint8_t base, negative_strand, mode, n_codes; uint32_t codes[4]; uint32_t rank_off, n_ranks; } mkp_host_tag;
int mkp_host_mm_ranks(const char* mm, uint32_t l_seq, uint32_t n_ml, mkp_host_tag* tags, uint32_t tags_cap, uint32_t* ranks, uint32_t ranks_cap);
int mkp_host_map_order(const uint32_t* code_reprs, uint32_t n, uint32_t* order_out);

#ifdef __cplusplus
}
#endif
#endif /* MKPILEUP_H */
