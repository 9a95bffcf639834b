// Structures shared by the host packer and the gfx950 kernels.
// Data layout in HBM for one shard (a reference window of one contig):
//   MkpReadHdr  hdr[n_reads]        64 B each, coordinate order
//   uint32      cigar[]             BAM cigar words (len<<4|op)
//   uint16      cigar16[]           the same ops in 16 bits (len<<4|op, len <= 4095: mkp_cigar_pack.hpp), each read at an offset of its own
//                                   that is a multiple of four entries; what mkp_decode_slots reads of a read without MKP_RF_CIGW
//   uint2       chunk_pfx[]         per read, per 64 CIGAR ops: query / reference offsets at the chunk start (the host walks the
//                                   CIGAR anyway to get the read's reference span), so a tile starts its walk at the right chunk
//   uint8       seq[]               BAM 4-bit packed bases, each read 4-byte aligned
//   MkpTagRef   tagref[]            one per MM tag of each read
//   uint32      ranks[]             per call: cumulative occurrence index of the tag's fundamental
//                                   base in the as-sequenced read (Σ(delta+1)-1, mod_bam.rs:697-733),
//                                   or the absolute forward position for `N` tags (735-767)
//   uint8       ml[]                ML qualities (bytes of the B:C array)
//   MkpLayout   layout[]            interned MM header structure + caller tables (host-built)
//   uint32      read_ids[]          reads by decode kernel class (FAST 1 tag | FAST 2 tags | general), longest first in a class
//   MkpEvent    events[]            written by the decode kernels, read by mkp_pileup_tiles
//   MkpReadOut  readout[n_reads]    per-read decode summary
//   MkpTile     tiles[n_tiles]      reference range + read range of every tile, genome order (host tile planner)
//   uint32      slotbm[]            focus runs only: one bit per reference position of the window (+64 positions of margin each
//                                   side), set where the position is in focus — the positions that get a tally column ("slot")
//   MkpRowsDev  rows                SoA row buffers (per tile, then gathered into genome order)
//   uint2       plane[]             slot pipeline: the call plane and, behind it, the base plane of the fused reads (MkpCallEnt, MkpBaseEnt,
//                                   MKP_PLANE_WORDS below), built once per resident shard
#pragma once
#include <stdint.h>

#define MKP_MAX_TAGS 8        // MM tags per read
#define MKP_KMAX 4            // distinct mod codes per (mod strand, base) group
#define MKP_MAX_MEMBERS 4     // tags per (mod strand, base) group
#define MKP_MAX_SLOTS 12      // distinct (primary base, code) pairs per run
#define MKP_MAX_COUNTERS (6 + 4 + MKP_MAX_SLOTS)
#define MKP_PAT_INFERRED 16   // pattern index of the all-inferred ('.' mode) case
#define MKP_HALO 16           // tile halo for strand combining (motif length <= 16)

// counter ids inside one strand tally (Tally, pileup/mod.rs:167-174)
#define MKP_C_NC 0            // NoCall(base) 0..3
#define MKP_C_DEL 4
#define MKP_C_FAIL 5
#define MKP_C_CAN 6           // + index of primary base among the run's primary bases; MOD ids follow

struct MkpReadHdr {
  int32_t ref_start, ref_end;
  uint32_t l_seq, n_cigar;
  uint32_t cigar_off;   // index into cigar[]
  uint32_t seq_off;     // byte offset into seq[]
  uint32_t tag_off;     // index into tagref[]
  uint16_t n_tags;
  uint16_t layout;
  uint32_t flags;       // bit0 reverse; bit1 host-detected tag error (coverage-only read); bit2 MKP_RF_SUMERR; bit5 MKP_RF_CIGW; bits 8.. partition key id (0 = ungrouped)
  uint32_t event_off;   // index into events[]
  uint32_t event_cap;
  uint32_t chunk_off;   // index into chunk_pfx[]: one {query offset, reference offset} per 64 CIGAR ops of this read
  // focus runs (slot pipeline, mkp_slots.hip): the read's focus positions ("slots") are the global slots [gs0, gs0 + n_sl) of
  // slot_pos[]; its features go to cov[cov_off .. cov_off + n_sl) (4-byte aligned).  Filled by the host planner (plan_slot_tiles, mkp_plan.hpp).
  uint32_t gs0, n_sl, cov_off;
  // index into cigar16[] (a multiple of 4; straight from the device ingest, bit 0 carries the probability-sum test until the host moves it
  // into dev_sum2).  `pad` is the field's name from before it had a use: the ingest test harness still reads it under that name.
  union { uint32_t cigar16_off; uint32_t pad; };
};
#define MKP_RF_REVERSE 1u
#define MKP_RF_BAD 2u
#define MKP_RF_SUMERR 4u   // host planner: some call's probabilities over the read's two tags add up to more than 1.01 (combine_checked, mod_bam.rs:629-656)
#define MKP_RF_RUNOVER 8u  // mkp_call_plane (work records only): the delta list runs past the last occurrence of its base (mod_bam.rs:705-727)
#define MKP_RF_SEQN 16u    // mkp_call_plane (work records only): the stored read holds a base that is not A/C/G/T (the decoder reads its SEQ)
#define MKP_RF_CIGW 32u    // both packers: some CIGAR op is longer than 4 095 bases (MKP_CIGAR16_MAX_LEN): the slot decoder reads the read's 32-bit CIGAR
#define MKP_RF_KEY_SHIFT 8
#define MKP_NO_KEY_FILTER 0xffffffffu

struct MkpTagRef { uint32_t rank_off, n, ml_off, pad; };

struct MkpEvent {  // the packed (ref_pos, strand, class, base) event of BASELINE.json's north_star
  uint32_t pos;
  uint32_t info;   // [0:7] counter id of the call class, [8] tally strand of the call,
                   // [9:10] read base, [11] alignment strand, [12] decrement NoCall(read base)
};

struct MkpReadOut { uint32_t n_events; uint32_t ok; uint32_t obs[2]; };  // obs: slot bitmask per tally strand

struct MkpTagDesc { uint8_t fb /*0..3, 4 = N*/, neg, mode /*0 ? 1 . 2 default*/, n_codes; };

struct MkpGroupDesc {          // one (mod strand σ, read base b) group; index σ*4+b.  128 bytes, dword-packed so a
                               // lane fetches everything it needs with a handful of independent LDS reads.
  uint32_t misc;               // [0:2] n_members, [3:6] implicit members (modes '.'/none, fb != N), [7:9] collapse local+1 (0 = none),
                               // [10:14] counter id of Canonical(threshold_base), [16:17] threshold_base, [20:22] n_codes
  uint32_t slots;              // 4 x 8 bit: local code -> global slot
  uint32_t cids;               // 4 x 8 bit: local code -> counter id of Modified(code)
  uint32_t member_tags;        // 4 x 4 bit: member -> tag index
  float thr_mod[MKP_KMAX];     // pass threshold per local code (threshold_mod_caller.rs:36-43)
  float thr_can;
  uint32_t pad[3];
  uint32_t pat[20];            // per hit pattern (1..15, 16 = all-inferred): [0:2] n_pre, [3:5] n_post,
                               // [8:15] FxHashMap iteration order before collapse (4 x 2 bit local idx), [16:23] after collapse
};
#define MKP_G_NMEM(m) ((m) & 7u)
#define MKP_G_IMPL(m) (((m) >> 3) & 15u)
#define MKP_G_COLL(m) ((int)(((m) >> 7) & 7u) - 1)
#define MKP_G_CIDCAN(m) (((m) >> 10) & 31u)
#define MKP_G_TB(m) (((m) >> 16) & 3u)

struct MkpLayout {
  uint8_t n_tags;
  uint8_t default_mask;   // tags whose mode is DefaultImplicitUnmodified
  uint8_t fast;           // 1: all tags share one specific base and mod strand and no code is listed twice (single group, distinct codes)
                          // 2: duplex — two such groups on different bases (`C+h?;C+m?;G-h?;G-m?`): the first `pad` tags form one, the rest the other
  uint8_t pad;            // fast == 2: tags in the first group
  MkpTagDesc tags[MKP_MAX_TAGS];
  uint32_t tagmap[MKP_MAX_TAGS][4];  // per (tag, read base): [0:3] member index in its group, [4+4i..] local code idx of the tag's i-th code
  uint32_t pad2[7];                  // groups start 16-byte aligned (offset 192)
  MkpGroupDesc groups[8];
};

#define MKP_LAYOUT_DWORDS 304
#define MKP_LAYOUT_GROUP_DW 48
#ifdef __cplusplus
static_assert(sizeof(MkpReadHdr) == 64, "read header is 16 dwords");
static_assert(sizeof(MkpGroupDesc) == 128, "group desc is 32 dwords");
static_assert(sizeof(MkpLayout) == 4 * MKP_LAYOUT_DWORDS, "layout is 304 dwords");
#endif

struct MkpSlot { uint32_t code_repr; uint8_t pb; uint8_t cid; uint8_t can_cid; uint8_t pad; };

struct MkpCombo {  // == mkp_motif_combo
  uint8_t n_pos, n_neg;
  uint8_t pos_ids[4], neg_ids[4];
  int8_t pos_delta[4];
  uint8_t pad[2];
};

// (Every kernel that takes this block — by value or through LDS — is compiled against its size: in round 5 one more dword here re-rolled
//  the register allocation of mkp_pileup_tiles into a build 8 % slower on the C2 workload.  After changing it, A/B the accumulate kernels
//  against the previous build on one box: tools/dbg/build_variant.sh + tools/dbg/r5_ab_lib.sh.)
struct MkpRunParams {
  // reference window
  int32_t win_start, win_end;
  uint32_t slot_cap, focus_words;   // S: tally columns per tile; W: bitmap words per tile (0 = no focus: slot = position)
  // counters
  uint32_t n_counters;      // per strand tally
  uint32_t n_slots;
  uint32_t n_pb;            // distinct primary bases with CAN counters
  uint32_t numeric_mode;    // 0 passthrough / 2 collapse (same row logic), 1 combine
  uint32_t combine_strands;
  uint32_t edge_filter, edge_start, edge_end, edge_inverted;
  uint32_t force_allow;
  uint32_t max_depth;
  uint32_t has_focus;
  uint32_t n_combos;
  uint32_t row_capacity;
  uint32_t sample_mode;     // 1: threshold sampling pass — emit argmax probabilities instead of call events
  uint32_t only_mapped;     // sampling: keep only calls with an aligned reference position
  // ablation only (-DMKP_DEBUG builds, env MKP_DEBUG_SKIP).  Tile kernels: 1 no depth walk, 2 no events (dense), 4 no rows, 8 no SEQ
  // phase (hemi); event decoders: 16, 32; slot pipeline: 64 ... 4096 (named where they are read)
  uint32_t debug_skip;
  uint8_t pb_of_can[4];     // CAN counter k -> primary base
  uint8_t can_of_pb[4];     // primary base -> CAN counter k or 0xff
  uint8_t slot_order[MKP_MAX_SLOTS];   // slots sorted by (code_repr, pb)
  MkpSlot slots[MKP_MAX_SLOTS];
  // pileup-hemi (duplex.rs): per '+' motif position and primary base, one counter per (positive-strand call, negative-strand call)
  // pattern.  A pattern element is 0 for a canonical call, 1.. for the base's mod codes in DuplexModCodeRepr order.
  uint32_t hemi;                          // 1: mkp_pileup_tiles_hemi tallies
  int32_t hemi_off;                       // MotifInfo::negative_strand_position: partner position = position + hemi_off
  uint32_t hemi_counters;                 // counters per tally column (MKP_H_* layout below)
  uint8_t hemi_pat_base[4];               // primary base -> its first pattern counter (0xff: the base has no calls in this run)
  uint8_t hemi_nel[4];                    // primary base -> pattern elements (1 + mod codes; 2 with --combine-mods)
  uint8_t hemi_el[MKP_MAX_COUNTERS + 2];  // call-event counter id -> pattern element; 0xff = Filtered
  uint32_t readout_b_off;                 // duplex reads decoded one group per wave: the second group's summary sits at readout[readout_b_off + read]
  uint32_t slot_stream;                   // 1: focus run on the slot pipeline (feature stream + mkp_pileup_stream)
};
// pileup-hemi counters of one tally column: NoCall(base) 0..3, deletions, Filtered(base) 5..8, then the pattern blocks
#define MKP_H_NC 0
#define MKP_H_DEL 4
#define MKP_H_FAIL 5
#define MKP_H_PAT 9
#define MKP_H_MAX_COUNTERS 64

// One tile of mkp_pileup_tiles: rows are emitted for reference positions [r0, r1) (inside the shard window); tallies are kept
// for the slots of [r0 - MKP_HALO, r1 + MKP_HALO) (strand combining reads a partner up to MKP_HALO away); reads [first, last)
// are the candidates overlapping that range.  A "slot" is a position that owns a tally column in LDS: every position of
// the range when the run has no focus (dense tiles), the '+' motif positions only for pileup-hemi.
struct MkpTile { int32_t r0, r1; uint32_t first, last; };
#define MKP_SLOTBM_MARGIN 64   // slot bitmap origin = win_start - MKP_SLOTBM_MARGIN

// mkp_pileup_tiles geometry: 16 waves per tile.  Dynamic LDS, in dwords:
//   tallies  [words_per_slot][S]            S = slot capacity of a tile (multiple of 64), 16-bit-packed strand tallies (wide shards:
//                                           words_per_slot doubled, one u32 plane per strand)
//   pileup-hemi (focus_words = W > 0): bm[W] + pfx[W] (slot bitmap of the tile's reference range and its running popcount),
//                                           fpos[S] (slot -> position)
//   per wave: dense = an op-start bitmap over the tile's slots (even number of dwords, 2 spare for the 64-bit window read) and a
//   64 x 8-byte compaction buffer; hemi = one word per slot of a read's visit (the packed query index / kind the CIGAR phase
//   leaves for the SEQ phase)
#ifndef MKP_PILEUP_THREADS
#define MKP_PILEUP_THREADS 1024
#endif
#define MKP_PILEUP_WAVE_SCRATCH 128
#define MKP_PILEUP_BM_WORDS(S) (((((S) + 31u) >> 5) + 3u) & ~1u)
#define MKP_PILEUP_WAVE_WORDS(S, focus_words) ((focus_words) && (S) > MKP_PILEUP_BM_WORDS(S) + MKP_PILEUP_WAVE_SCRATCH ? (S) : MKP_PILEUP_BM_WORDS(S) + MKP_PILEUP_WAVE_SCRATCH)
#define MKP_PILEUP_LDS_WORDS(words_per_slot, S, focus_words) ((words_per_slot) * (S) + ((focus_words) ? 2u * (focus_words) + (S) : 0u) + (MKP_PILEUP_THREADS / 64) * MKP_PILEUP_WAVE_WORDS(S, focus_words))

// ---- slot pipeline (focus runs: --cpg / --motif / --include-bed; mkp_slots.hip) -------------------------------------------
// The decode side leaves one FEATURE BYTE per (read, focus position in the read's reference span) — position-implicit: byte k
// of a read belongs to global slot gs0 + k — and one MkpVisit per read; mkp_pileup_stream is then a pure histogram of that
// stream into LDS tallies.  Feature byte = what FeatureVector::add_feature receives for this alignment at this column
// (pileup/mod.rs:783-939): [0:4] counter id (MKP_C_*), [5] tally strand, [6:7] the read base as tallied (so that a call of a
// record that later fails can be counted as NoCall(base)).
// mkp_decode_slots takes whether a call is listed under a slot, and the base where none is, from TWO PLANES (mkp_call_plane, built once
// when the shard becomes resident), each with one 8-byte entry per fused read and 32 stored bases, stored order: the CALL PLANE (one bit
// per base, and the calls before the entry) and, behind the whole of it in the same buffer, the BASE PLANE (two bits per base).  A read's
// entries start at index MkpWork.pad of either plane.  A slot with a listed call never needs its base (the call's feature replaces the
// coverage feature), so a read with calls gathers its call entries and asks the base plane for one dword only under a match slot without a
// listed call; every other read gathers its base entries and never touches the call plane.  A read whose SEQ holds a base that is not
// A/C/G/T (MKP_RF_SEQN) has code 0 there: the decoder reads such a read's bases from the SEQ instead.
#define MKP_PLANE_WORDS(l_seq) (((l_seq) + 31u) >> 5)
struct MkpCallEnt {          // 8 B: one global_load_dwordx2 per slot of a read with calls
  uint32_t listed;           // bit b = a listed call of the read sits at base 32 w + b (0 for a read without calls or a run-over list)
  uint32_t before;           // listed calls at the bases before 32 w
};
struct MkpBaseEnt {          // 8 B: one global_load_dwordx2 per slot of a read without calls; a read with calls loads the half that holds its base
  uint32_t base_lo, base_hi; // 2-bit codes of stored bases 32 w + b (A=0 C=1 G=2 T=3, not complemented): b < 16 at bits 2 b of base_lo,
                             // b >= 16 at bits 2 (b - 16) of base_hi (mkp_pack_bases32, mkp_base_pack.hpp)
};
#define MKP_STREAM_ROWMAP_WORDS 2048u   // mkp_pileup_stream: rows of a tile placed per emission round (a dword of LDS each)
// one entry of the slot-entry lists (`all`, `plus`, `minus`, concatenated: window_slots, mkp_plan.hpp): the decoder's 8-byte load per slot
struct MkpSlotEnt { uint32_t pos, g; };   // reference position, global slot index (its place in slot_pos[])
#define MKP_FB_NONE 0xffu    // the read is not in this column (ref-skip)
#define MKP_FB_BLANK 0xfeu   // in the column, no feature (non-ACGT base: pileup/mod.rs:864-874)
struct MkpVisit {            // 32 B, written by the decode / cover kernels, read by mkp_pileup_stream
  uint32_t gs0, n_sl, cov_off;
  uint32_t flags;            // bit0 record yielded calls (observed-code masks valid), bit1 alignment strand, bit2 stream holds NONE bytes,
                             // bits 8.. partition key id
  uint32_t obs0, obs1;       // observed-code slot masks per tally strand (read_cache.rs:171-194)
  uint32_t over_off, n_over; // second features on one column (pos_call and neg_call at one base): {global slot, feature byte} pairs in events[]
};
// what mkp_decode_slots* needs of a layout whose tags form one explicit-mode group (decode class SPARSE), resolved by the host from
// the MkpLayout so that a wave gets it with one scalar load: the caller's walk over a call's map in iteration order
struct MkpFusedDesc {        // 64 B
  uint32_t misc;             // [0:1] fundamental base, [2] mod strand, [3:5] codes the caller sees (n_post), [6] / [7] the integer form of the caller is exact
                             // without / with the collapse, [8:15] counter of Canonical, [16:31] observed-code slot mask
  uint32_t it_cid;           // 4 x 8 bit: counter of Modified(i-th code)
  uint32_t it_src;           // 4 x 4 bit: where the i-th code's ML byte sits: [0] tag, [1:3] index among the tag's codes
  uint32_t nc;               // codes per call of tag 0 | tag 1 << 8 (the tags' ML strides)
  float it_thr[4];           // pass threshold of the i-th code
  float thr_can;
  // --ignore / --preset traditional: ReDistribute(x) (BaseModProbs::into_collapsed, mod_bam.rs:558-600) — when the map holds x, every
  // other code gets p_x / n_other added (n_other = number of codes before the collapse; x is no longer among the it_* entries)
  uint32_t col;              // [0] the map holds x, [1:4] where x's ML byte sits (tag | index << 1), [5:6] log2(n_other) when it is 1, 2 or 4
  float n_other;
  // The caller in integers (round 6).  (q + 0.5) / 256 is a multiple of 2^-9 and, when n_other is a power of two, so is every value the
  // f32 walk forms — shares, sums, 1 - sum — a multiple of 2^-11 that f32 holds exactly: `p >= threshold` is `p * 2048 >= i_thr` with
  // i_thr = the least integer T such that T / 2048 >= threshold (INT32_MAX for a NaN threshold: never passed).
  int32_t i_can;
  int32_t i_thr[4];          // (16-byte aligned: one LDS vector read per slot batch)
};
static_assert(sizeof(MkpFusedDesc) == 64, "MkpFusedDesc is one 64-byte scalar load");
// one read as mkp_decode_slots* takes it: the header and tag fields the kernel needs, in launch order (longest reads first), so that a
// wave starts from ONE 64-byte scalar load instead of the chain read id -> header -> tag table
struct MkpWork {             // 72 B
  // cigar_off: index into cigar16[] (the header's cigar16_off), into cigar[] for a read with MKP_RF_CIGW
  int32_t ref_start; uint32_t l_seq, n_cigar, cigar_off, seq_off, flags, gs0, n_sl, cov_off;
  uint16_t n_tags, layout;
  uint32_t rank_off, n_calls, ml_off0, ml_off1;   // the shared rank list, the tags' ML bytes
  uint32_t rid, pad;                              // pad: the read's first entry in either plane (MKP_PLANE_WORDS(l_seq) of them)
  // the slots the decoder visits: slot_ent[ent_off .. ent_off + n_ent), the read's run of the slot-entry list of its own strand — or of
  // the list of every slot (n_ent == n_sl) when it needs both tally strands or its strand's list is no shorter (plan_read_entries, mkp_plan.hpp)
  uint32_t ent_off, n_ent;
};
// Records that share a read NAME inside one interval of the reference's grid (unmarked duplicates, mates, split reads that kept the primary flag).
// The reference keeps ONE cache entry per name and interval (ReadCache, read_cache.rs:24-43): the record asked about first — the first focus
// column of the interval that holds a record of the name, file order within a column — is parsed; every later record of the name is answered
// from THAT record's call map, looked up by reference position and the asking record's own read base (get_mod_call, 232-297).  The host planner
// works out, per interval, which record owns the name (plan_name_owners, mkp_plan.hpp); a record that is answered from another one in some interval is a
// CONSUMER: mkp_dup_events rebuilds its event list — its own events where it owns the name, the owner's events elsewhere, kept where its own
// alignment shows the call's base — and the accumulate kernels then take that list as the record's own.
// positions [p_lo, p_hi) of one consumer, ascending
struct MkpDupSeg { int32_t p_lo, p_hi; uint32_t src_off /* the owner's OWN event slice */, owner; };
struct MkpDupCons {
  uint32_t rid, seg_off, n_seg;
  uint32_t own_off;    // the record's own event slice (what its decode kernel writes)
  uint32_t eff_off, eff_cap;   // the rebuilt list
  uint32_t out_n, out_ok, out_obs0, out_obs1;   // written by mkp_dup_events, moved into the record's header / summary by mkp_dup_apply
  uint32_t pad[6];
};
// the error word of a pass (the kernels' dev_err; mkp_launch.h says where it lies)
#define ERR_EVENT_CAP 1u   // device error bit: a read's events (a sampling pass: the sampled values) outgrew their slice
#define ERR_ROW_CAP 2u     // device error bit: the rows outgrew row_capacity (the host doubles it and runs the pass again)
#define ERR_DEPTH 4u       // (no kernel raises it)
#define ERR_DUP_MIXED 8u   // device error bit: the records a consumer is answered from disagree in status or observed codes (refused, not approximated)
#define MKP_VF_OK 1u
#define MKP_VF_REV 2u
#define MKP_VF_GAPS 4u
// one tile of mkp_pileup_stream: rows for the global slots [g0, g1) (positions [r0, r1)), tally columns for [gh0, gh1) (+- MKP_HALO
// positions for strand combining), candidate reads [first, last)
struct MkpSTile { uint32_t g0, g1, gh0, gh1; int32_t r0, r1; uint32_t first, last; };

// one BGZF block of an inflate launch (mkp_inflate_wave4.hip; mkp_crc32_blocks and mkp_bgzf_layout of mkp_ingest.hip): where its DEFLATE
// payload lies in the compressed bytes and where its inflated bytes go
struct MkpBgzfBlock { unsigned long long in_off; unsigned long long out_off; uint32_t in_len; uint32_t out_len; };

struct MkpRowsDev {  // SoA row buffers (44 B / row)
  uint32_t* pos; uint32_t* info; uint32_t* code;
  uint32_t* n_valid; uint32_t* n_mod; uint32_t* n_can; uint32_t* n_other;
  uint32_t* n_del; uint32_t* n_fail; uint32_t* n_diff; uint32_t* n_nocall;
};
// ---- region statistics (mkp_stats.hip): a region of the contig whose rows are being added, and where its totals go.  The run-long
// table holds MKP_STATS_MAX_CODES slots of {n_mod, n_valid} (u64) per region, a 32-bit mask of the slots with a counted row per region,
// and the code of every slot (0 = free) in a table of its own.
#define MKP_STATS_CHUNK 4096u       // rows per (region, chunk) work item of mkp_stats_reduce
#define MKP_STATS_MAX_CODES 16      // distinct mod codes per run (the pileup itself allows MKP_MAX_SLOTS (base, code) pairs)
#define MKP_STATS_ERR_CODES 1u      // device error bit: a seventeenth code
struct MkpStatsRegion { uint32_t start, end; uint32_t rule /* 1 '+', 2 '-', 3 both */; uint32_t out /* index into the run's table */; };
// ---- dmr pair (mkp_dmr.hip): regions as MkpStatsRegion (`out` = the region's line of one sample's table).  A line holds MKP_DMR_CELLS
// u64: the sum of N_mod per code slot, then the total (the N_valid_cov of every good position once) and the participating rows; beside
// it a 32-bit mask per line: bit s = a participating row of slot s, MKP_DMR_SEEN_BAD = an inconsistent position.
#define MKP_DMR_CELLS (MKP_STATS_MAX_CODES + 2)
#define MKP_DMR_CELL_TOTAL MKP_STATS_MAX_CODES
#define MKP_DMR_CELL_ROWS (MKP_STATS_MAX_CODES + 1)
#define MKP_DMR_SEEN_BAD 0x80000000u
#define MKP_DMR_MAX_LOOKUP 64       // entries of the code -> base table (the reference's own holds 17)
// base sets: bit b of a set = base b of "ACGT"; base[k] = the index in "ACGT" of the base code[k] modifies; mask != 0: a lower-case
// reference byte is no base (--mask), otherwise it counts as its upper-case form
struct MkpDmrParams { unsigned long long min_cov; uint32_t n_lookup, pos_set, neg_set, mask; uint32_t code[MKP_DMR_MAX_LOOKUP];
  uint8_t base[MKP_DMR_MAX_LOOKUP]; };
// ---- dmr sites (mkp_dmr_sites.hip): the rows of one contig of one sample are cut into tiles of MKP_DMRS_TILE rows, a workgroup each, a
// lane a row.  A row's flag byte: its code slot, whether it takes part, whether it is the head (first participating row) of its position.
// A site = the participating rows of a position: its pos, first row, total (the head's N_valid_cov) and info bits.  A contig's batch table
// lists, ascending in start, where each batch of the reference's walk begins inside it.
#define MKP_DMRS_TILE 256u
#define MKP_DMRS_ROW_SLOT 0x0fu
#define MKP_DMRS_ROW_PART 0x20u
#define MKP_DMRS_ROW_HEAD 0x40u
#define MKP_DMRS_SITE_MINUS 1u      // site info: listed '-'
#define MKP_DMRS_SITE_BAD 2u        // site info: aggregate_counts fails on the position
#define MKP_DMRS_NO_PAIR 0xffffffffu
#define MKP_DMRS_PAIR_FAILED 2u     // pair info (beside MKP_DMRS_SITE_MINUS): the score or the p-value fails in the reference
struct MkpDmrSitesBatch { uint32_t start, batch; };
// one sample's rows and sites of the contig, as the score kernel reads them
struct MkpDmrSitesSample { const uint32_t *pos, *n_mod; const uint8_t* rowflag; uint32_t n_rows; const uint32_t *s_pos, *s_first, *s_total, *s_info; };
// per pair: pos, info (MKP_DMRS_SITE_MINUS | MKP_DMRS_PAIR_FAILED), has = a's column mask | b's << 16, the totals, cnt[(pair * 2 + sample) *
// n_cols + column], and the three f64 values
struct MkpDmrSitesPairs { uint32_t *pos, *info, *has, *total_a, *total_b, *cnt; double *score, *pvalue, *effect; };
// ---- dmr replicates (mkp_dmr_reps.hip): up to MKP_DMRR_MAX_SIDE samples a side, each with its rows and sites as dmr sites makes them.  A side's
// site set of a contig is a bitmap of one bit a position; a joined site = a position at least one sample of each side holds, outside the
// dropped batches.
#define MKP_DMRR_MAX_SIDE 16u
#define MKP_DMRR_SITE_OVERFLOW 4u   // joined-site info (beside MKP_DMRS_SITE_MINUS and MKP_DMRS_PAIR_FAILED): a summed total beyond 2^32 - 1
struct MkpDmrRepsSample { MkpDmrSitesSample s; uint32_t n_sites, pad; };
// per joined site: pos, info, present = a's sample mask | b's << 16, pct = the two shares of samples likewise, has = the column masks likewise;
// total / bal_total[site * 2 + side]; cnt / bal_cnt[(site * 2 + side) * n_cols + column] (collapsed and balanced counts); msum[site * 4 + ..] =
// the modified counts {collapsed a, collapsed b, balanced a, balanced b}; rep[((site * 2 + side) * rep_stride + rank) * 2 + ..] = {modified,
// total} of the side's present samples by rank (matched runs only: rep_stride = the samples a side, otherwise 0 and the rep arrays unused);
// the f64 values, rep_pvalue / rep_effect[site * rep_stride + rank] for rank < n_rep[site]
struct MkpDmrRepsSites { uint32_t *pos, *info, *present, *pct, *has, *total, *bal_total, *cnt, *bal_cnt, *msum, *rep, *n_rep;
  double *score, *pvalue, *effect, *bal_pvalue, *bal_effect, *rep_pvalue, *rep_effect; };
// ---- localize (mkp_localize.hip): one expanded window [ws, we) of the contig whose rows are being added and the anchor its offsets are
// taken from (offset = anchor - pos).  The run-long table holds MKP_STATS_MAX_CODES slots of 2 * window + 1 cells {n_mod, n_valid, n_rows}
// (u64 each); the codes of the slots (0 = free) are a table of the run's own.
#define MKP_LOC_TILE 512u           // offsets per tile: a workgroup of mkp_localize_reduce keeps [MKP_LOC_LOCAL][MKP_LOC_TILE] cells in LDS
#define MKP_LOC_LOCAL 4             // code slots with cells in LDS; a row of a later slot adds to HBM directly
#define MKP_LOC_BATCH 256u          // regions per batch = threads per workgroup
#define MKP_LOC_MAX_WINDOW 100000u
struct MkpLocRegion { uint32_t ws, we, anchor; uint32_t rules /* fetch rule | region rule << 8, each 1 '+', 2 '-', 3 both */; };
// ---- bedmethyl merge (mkp_merge.hip): the output is cut into tiles at the merge-path diagonals k * MKP_MERGE_TILE, each cut moved back to
// the start of the position it lands in; a workgroup sorts up to MKP_MERGE_CAP rows in LDS (16 B a row: 32 KiB).  A tile is its
// MKP_MERGE_TILE rows plus what the position at its front holds behind the diagonal, so with the step a little under half the capacity
// most tiles sort 1024 entries and a single position may hold up to MKP_MERGE_CAP - MKP_MERGE_TILE rows.
#define MKP_MERGE_TILE 960u
#define MKP_MERGE_CAP 2048u
struct MkpMergeCut { uint32_t a, b; };   // rows of the table / of the added rows in front of a tile
#define MKP_MERGE_ERR_TILE 1u       // device error bit: one position holds more rows than a tile has room for
#define MKP_MERGE_ERR_SUM 2u        // device error bit: a summed count does not fit in 32 bits
// ---- device bedMethyl reader (mkp_bedmethyl.hip): a piece of text is cut into chunks of MKP_BEDIN_CHUNK bytes, a workgroup each, a lane
// 16 bytes.  The piece's words (dwords of one small buffer; the host zeroes them in front of a piece, MKP_BEDIN_W_ERR_OFF to all ones):
#define MKP_BEDIN_CHUNK 4096u
enum {
  MKP_BEDIN_W_LINES = 0,       // data lines that start in the piece, the unfinished one behind its last line end included
  MKP_BEDIN_W_LAST_NL = 1,     // the offset behind the piece's last '\n' (0: the piece holds none)
  MKP_BEDIN_W_NL = 2,          // '\n' bytes of the piece: its physical lines
  MKP_BEDIN_W_ROWS = 3,        // data lines that end in the piece: its rows
  MKP_BEDIN_W_LIMIT = 4,       // where the last of them ends: LAST_NL, or the piece's length when it is the file's last
  MKP_BEDIN_W_ERR = 5,         // MKP_BEDIN_ERR_* bits
  MKP_BEDIN_W_RUNS = 6,        // contig runs of the piece
  MKP_BEDIN_W_NAME_BYTES = 7,  // bytes of their names
  MKP_BEDIN_W_ERR_OFF = 8,     // u64: the least offset of a line with an error bit
  MKP_BEDIN_W_FIRST_POS = 10, MKP_BEDIN_W_LAST_POS = 11,   // pos of the first and of the last row (the host checks the order across a seam)
  MKP_BEDIN_WORDS = 16
};
#define MKP_BEDIN_ERR_PARSE 1u      // a line does not parse
#define MKP_BEDIN_ERR_RANGE 2u      // a decimal field beyond 2^32 - 1
#define MKP_BEDIN_ERR_ORDER 4u      // pos descends inside a contig run
#define MKP_BEDIN_ERR_LONG 8u       // a line longer than a piece may hold
struct MkpBedRun { uint32_t row, name_off, name_len; };   // a contig run: its first row, its name's bytes in the names buffer
#ifdef __cplusplus
static_assert(sizeof(MkpWork) == 72 && sizeof(MkpSlotEnt) == 8, "work record is 18 dwords");
static_assert(sizeof(MkpFusedDesc) == 64 && sizeof(MkpVisit) == 32 && sizeof(MkpCallEnt) == 8 && sizeof(MkpBaseEnt) == 8, "slot pipeline records");
#endif
