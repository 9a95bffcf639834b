"""modkit_amd — Python host mirror of libmkpileup (the MI355X implementation of `modkit pileup`).

The product is the C-ABI shared library built from modkit_amd/csrc (include/mkpileup.h); this module
only loads it and mirrors the reference's `modkit pileup` command surface:

    modkit_amd.pileup(["in.bam", "out.bed", "--cpg", "--ref", "ref.fa", ...])   # == `modkit pileup ...`

There is no CPU path: every call runs the HIP kernels and fails loudly when the library or a gfx950
device is missing.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("MKP_LIB_PATH") or os.path.join(CSRC, "libmkpileup.so")   # MKP_LIB_PATH: another build of the same library (e.g. -DMKP_DEBUG ablations)

MKP_OK = 0
STATUS = {0: "MKP_OK", -1: "MKP_E_INVALID", -2: "MKP_E_IO", -3: "MKP_E_UNSUPPORTED", -4: "MKP_E_DEVICE", -5: "MKP_E_NOMEM",
          -6: "MKP_E_THRESHOLD"}


class MkpError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (STATUS.get(status, status), message))
        self.status = status


def build(force=False):
    """Compile libmkpileup.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-C", CSRC, "libmkpileup.so", "mkpileup"])
    return LIB_PATH


_lib = None


def lib():
    """The loaded library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MkpError(-4, "libmkpileup.so is not built (run modkit_amd.build() / __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        L.mkp_version.restype = ctypes.c_char_p
        L.mkp_host_threads.restype = ctypes.c_uint
        L.mkp_last_error.restype = ctypes.c_char_p
        L.mkp_last_error.argtypes = [ctypes.c_void_p]
        L.mkp_pileup_main.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_char_p, ctypes.c_size_t]
        L.mkp_ctx_create.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        L.mkp_ctx_destroy.argtypes = [ctypes.c_void_p]
        L.mkp_set_caller.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mkp_estimate_thresholds.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p]
        L.mkp_process_region.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
        L.mkp_shard_rerun.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        L.mkp_get_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mkp_pileup_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p]
        L.mkp_pileup_run_cb.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), THRESHOLD_FN, ctypes.c_void_p, ctypes.c_void_p]
        L.mkp_pileup_hemi_main.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_char_p, ctypes.c_size_t]
        L.mkp_extract_calls_main.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_char_p, ctypes.c_size_t]
        L.mkp_pileup_hemi_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p]
        L.mkp_summary.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p]
        L.mkp_bgzf_inflate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
        L.mkp_hemi_shard_run.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_void_p]
        u64p, f32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_float)
        L.mkp_sample_probs.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), f32p, ctypes.c_uint32, f32p, ctypes.c_void_p, u64p]
        L.mkp_histogram_begin.argtypes = [ctypes.c_void_p]
        L.mkp_histogram_add_bam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]
        L.mkp_histogram_get.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p]
        L.mkp_histogram_allreduce.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p]
        L.mkp_histogram_from_values.argtypes = [f32p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p]
        L.mkp_histogram_locate.argtypes = [u64p, ctypes.c_float, ctypes.POINTER(ctypes.c_uint32), u64p, u64p]
        L.mkp_histogram_resolve.argtypes = [ctypes.c_uint32, u64p, ctypes.c_uint64, f32p]
        L.mkp_percentile_from_histogram.argtypes = [ctypes.c_uint64, ctypes.c_float, ctypes.c_float, ctypes.c_float, f32p]
        if hasattr(L, "mkp_stats_begin"):   # (absent from an older build loaded through MKP_LIB_PATH)
            L.mkp_stats_begin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint64]
            L.mkp_stats_add_resident.argtypes = [ctypes.c_void_p]
            L.mkp_stats_add_rows.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
            L.mkp_stats_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.mkp_set_partition_tags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32]
            L.mkp_host_parse_regions.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_size_t]
            L.mkp_region_set_size.argtypes = [ctypes.c_void_p]
            L.mkp_region_set_size.restype = ctypes.c_uint32
            L.mkp_region_set_regions.argtypes = [ctypes.c_void_p]
            L.mkp_region_set_regions.restype = ctypes.POINTER(Region)
            L.mkp_region_set_chrom.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
            L.mkp_region_set_chrom.restype = ctypes.c_char_p
            L.mkp_region_set_name.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
            L.mkp_region_set_name.restype = ctypes.c_char_p
            L.mkp_region_set_free.argtypes = [ctypes.c_void_p]
            L.mkp_region_set_free.restype = None
            L.mkp_host_stats_table.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p]
        if hasattr(L, "mkp_localize_begin"):
            L.mkp_localize_begin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
            L.mkp_localize_add_resident.argtypes = [ctypes.c_void_p]
            L.mkp_localize_add_rows.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
            L.mkp_localize_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.mkp_localize_tile_offsets.argtypes = []
            L.mkp_localize_tile_offsets.restype = ctypes.c_uint32
            L.mkp_host_parse_localize_regions.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p),
                                                          ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_size_t]
            L.mkp_host_parse_genome_sizes.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_size_t]
            L.mkp_genome_sizes_size.argtypes = [ctypes.c_void_p]
            L.mkp_genome_sizes_size.restype = ctypes.c_uint32
            L.mkp_genome_sizes_name.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
            L.mkp_genome_sizes_name.restype = ctypes.c_char_p
            L.mkp_genome_sizes_length.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
            L.mkp_genome_sizes_length.restype = ctypes.c_uint64
            L.mkp_genome_sizes_free.argtypes = [ctypes.c_void_p]
            L.mkp_genome_sizes_free.restype = None
            L.mkp_host_localize_table.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        if hasattr(L, "mkp_merge_begin"):
            L.mkp_merge_begin.argtypes = [ctypes.c_void_p, u64p, ctypes.c_uint32]
            L.mkp_merge_add_rows.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
            L.mkp_merge_add_resident.argtypes = [ctypes.c_void_p]
            L.mkp_merge_get.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, u64p]
            L.mkp_merge_tile_rows.argtypes = []
            L.mkp_merge_tile_rows.restype = ctypes.c_uint32
            L.mkp_host_read_bedmethyl.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_size_t]
            L.mkp_bedmethyl_file_runs.argtypes = [ctypes.c_void_p]
            L.mkp_bedmethyl_file_runs.restype = ctypes.c_uint32
            L.mkp_bedmethyl_file_chrom.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
            L.mkp_bedmethyl_file_chrom.restype = ctypes.c_char_p
            L.mkp_bedmethyl_file_rows.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
            L.mkp_bedmethyl_file_free.argtypes = [ctypes.c_void_p]
            L.mkp_bedmethyl_file_free.restype = None
            L.mkp_merge_add_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, u64p]
            L.mkp_bedmethyl_read_device.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
            L.mkp_bedmethyl_chunk_bytes.argtypes = []
            L.mkp_bedmethyl_chunk_bytes.restype = ctypes.c_uint32
            L.mkp_bedmethyl_merge_main.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), u64p, u64p, ctypes.c_char_p, ctypes.c_size_t]
        if hasattr(L, "mkp_dmr_begin"):
            u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
            L.mkp_dmr_default_lookup.argtypes = [u32p, u8p, ctypes.c_uint32]
            L.mkp_dmr_default_lookup.restype = ctypes.c_uint32
            L.mkp_dmr_begin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, u32p, u8p, ctypes.c_uint32,
                                        ctypes.c_uint64, ctypes.c_int]
            L.mkp_dmr_set_reference.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
            L.mkp_dmr_add_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p]
            L.mkp_dmr_add_file.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, u64p]
            L.mkp_dmr_add_resident.argtypes = [ctypes.c_void_p, ctypes.c_int]
            L.mkp_dmr_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.mkp_host_parse_dmr_regions.argtypes = L.mkp_host_parse_regions.argtypes
            L.mkp_host_dmr_judge.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), u8p]
            L.mkp_host_dmr_table.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p]
            L.mkp_dmr_pair_main.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), u64p, ctypes.c_char_p, ctypes.c_size_t]
        if hasattr(L, "mkp_dmr_sites_begin"):
            u32p, f64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
            L.mkp_dmr_sites_begin.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.mkp_dmr_sites_set_reference.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_uint64]
            L.mkp_dmr_sites_add_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p]
            L.mkp_dmr_sites_add_file.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, u64p]
            L.mkp_dmr_sites_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.mkp_host_dmr_site_score.argtypes = [u64p, ctypes.c_uint32, ctypes.c_uint64, u64p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                                  ctypes.c_double, ctypes.c_double, ctypes.c_double, u32p, f64p, ctypes.POINTER(ctypes.c_int)]
            L.mkp_host_dmr_sites_batches.argtypes = [u64p, u32p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, u64p]
            L.mkp_host_dmr_sites_gauss_legendre.argtypes = [f64p, f64p]
            L.mkp_host_dmr_sites_table.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p]
            L.mkp_dmr_sites_main.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), u64p, ctypes.c_char_p, ctypes.c_size_t]
        if hasattr(L, "mkp_dmr_reps_begin"):
            u32p = ctypes.POINTER(ctypes.c_uint32)
            L.mkp_dmr_reps_begin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
            L.mkp_dmr_reps_set_reference.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_uint64]
            L.mkp_dmr_reps_add_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p]
            L.mkp_dmr_reps_add_file.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, u64p]
            L.mkp_dmr_reps_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.mkp_host_dmr_reps_balance.argtypes = [u64p, u32p, u64p, ctypes.c_uint32, ctypes.c_uint32, u64p, u32p, u64p, ctypes.POINTER(ctypes.c_int)]
            L.mkp_host_dmr_reps_pct.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
            L.mkp_host_dmr_reps_pct.restype = ctypes.c_uint32
            L.mkp_host_dmr_reps_table.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p]
            L.mkp_dmr_reps_main.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), u64p, ctypes.c_char_p, ctypes.c_size_t]
        # the structs this binding allocates mirror ONE revision of include/mkpileup.h: a library of another revision would write past them
        if os.environ.get("MKP_LIB_PATH") and not hasattr(L, "mkp_abi_version"):
            _lib = L   # (A/B runs against a build from before the query existed, tools/dbg/ab.sh)
            return _lib
        L.mkp_abi_version.restype = ctypes.c_uint32
        L.mkp_run_report_size.restype = ctypes.c_size_t
        if L.mkp_abi_version() != ABI_VERSION or L.mkp_run_report_size() != ctypes.sizeof(RunReport):
            raise MkpError(-1, "libmkpileup.so has ABI revision %d (mkp_run_report %d bytes), this binding %d (%d bytes): rebuild" %
                           (L.mkp_abi_version(), L.mkp_run_report_size(), ABI_VERSION, ctypes.sizeof(RunReport)))
        _lib = L
    return _lib


ABI_VERSION = 5   # MKP_ABI_VERSION of include/mkpileup.h
READ_WIDE_CIGAR = 32   # MKP_READ_WIDE_CIGAR


# mkp_threshold_fn (include/mkpileup.h): int fn(void* user, mkp_ctx* ctx, int have_sample, float thresholds[4], uint8_t has[4])
THRESHOLD_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8))

EXPORTS = ["mkp_ctx_create", "mkp_ctx_destroy", "mkp_last_error", "mkp_version", "mkp_abi_version", "mkp_run_report_size", "mkp_host_threads", "mkp_set_caller", "mkp_shard_begin",
           "mkp_shard_add_records", "mkp_shard_set_intervals", "mkp_shard_run", "mkp_batch_run", "mkp_shard_rerun", "mkp_get_stats", "mkp_shard_read_flags", "mkp_process_region", "mkp_pileup_main",
           "mkp_pileup_run", "mkp_pileup_run_cb", "mkp_percentile", "mkp_estimate_thresholds", "mkp_host_mm_ranks", "mkp_host_map_order",
           "mkp_set_partition_tags", "mkp_histogram_begin", "mkp_histogram_add_bam", "mkp_histogram_get", "mkp_histogram_allreduce", "mkp_histogram_from_values", "mkp_histogram_locate",
           "mkp_histogram_resolve", "mkp_percentile_from_histogram", "mkp_hemi_shard_run", "mkp_pileup_hemi_main", "mkp_pileup_hemi_run", "mkp_bgzf_inflate", "mkp_sample_probs", "mkp_summary", "mkp_extract_calls_main",
           "mkp_stats_begin", "mkp_stats_add_resident", "mkp_stats_add_rows", "mkp_stats_get", "mkp_host_parse_regions", "mkp_region_set_size",
           "mkp_region_set_chrom", "mkp_region_set_name", "mkp_region_set_free", "mkp_host_stats_table",
           "mkp_localize_begin", "mkp_localize_add_resident", "mkp_localize_add_rows", "mkp_localize_get", "mkp_localize_tile_offsets",
           "mkp_host_parse_localize_regions", "mkp_host_parse_genome_sizes", "mkp_genome_sizes_size", "mkp_genome_sizes_name",
           "mkp_genome_sizes_free", "mkp_host_localize_table",
           "mkp_merge_begin", "mkp_merge_add_rows", "mkp_merge_add_resident", "mkp_merge_get", "mkp_merge_tile_rows", "mkp_host_read_bedmethyl",
           "mkp_bedmethyl_file_runs", "mkp_bedmethyl_file_chrom", "mkp_bedmethyl_file_rows", "mkp_bedmethyl_file_free", "mkp_bedmethyl_merge_main",
           "mkp_merge_add_file", "mkp_bedmethyl_read_device", "mkp_bedmethyl_chunk_bytes",
           "mkp_dmr_default_lookup", "mkp_dmr_begin", "mkp_dmr_set_reference", "mkp_dmr_add_rows", "mkp_dmr_add_file", "mkp_dmr_add_resident", "mkp_dmr_get",
           "mkp_host_parse_dmr_regions", "mkp_host_dmr_judge", "mkp_host_dmr_table", "mkp_dmr_pair_main",
           "mkp_dmr_sites_begin", "mkp_dmr_sites_set_reference", "mkp_dmr_sites_add_rows", "mkp_dmr_sites_add_file", "mkp_dmr_sites_get",
           "mkp_host_dmr_site_score", "mkp_host_dmr_sites_batches", "mkp_host_dmr_sites_gauss_legendre", "mkp_host_dmr_sites_table", "mkp_dmr_sites_main",
           "mkp_dmr_reps_begin", "mkp_dmr_reps_set_reference", "mkp_dmr_reps_add_rows", "mkp_dmr_reps_add_file", "mkp_dmr_reps_get",
           "mkp_host_dmr_reps_balance", "mkp_host_dmr_reps_pct", "mkp_host_dmr_reps_table", "mkp_dmr_reps_main"]   # (mkp_genome_sizes_length returns a uint64_t, as mkp_region_set_regions a pointer: not listed)


def pileup(argv):
    """`modkit pileup` (ModBamPileup::run, src/pileup/subcommand.rs:382): argv = [in_bam, out_bed, flags...]."""
    L = lib()
    args = [str(a).encode() for a in argv]
    arr = (ctypes.c_char_p * len(args))(*args)
    err = ctypes.create_string_buffer(2048)
    rc = L.mkp_pileup_main(len(args), arr, err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    return rc


def pileup_hemi(argv):
    """`modkit pileup-hemi` (DuplexModBamPileup::run, src/pileup/subcommand.rs:1122): argv = [in_bam, "-o", out_bed, flags...]."""
    L = lib()
    args = [str(a).encode() for a in argv]
    arr = (ctypes.c_char_p * len(args))(*args)
    err = ctypes.create_string_buffer(2048)
    rc = L.mkp_pileup_hemi_main(len(args), arr, err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    return rc


def bedmethyl_merge(argv):
    """`modkit bedmethyl merge` (EntryMergeBedMethyl::run, src/bedmethyl_util/subcommands.rs:198-371) on the device: argv = [a.bed, b.bed, ...,
    "-g", sizes.tsv, "-o", out.bed, "--force", "--bgzf"]; the inputs are bedMethyl tables, plain text or bgzip compressed (its own --bgzf output
    included; a .tbi is not needed), each read by the device reader (Context.merge_add_file; MKP_HOST_BEDMETHYL=1: by the host reader).
    Returns (rows written, rows dropped): a row is dropped when its contig is not in the sizes file or its start is not below the contig's
    length."""
    L = lib()
    args = [str(a).encode() for a in argv]
    arr = (ctypes.c_char_p * max(1, len(args)))(*args)
    err = ctypes.create_string_buffer(2048)
    written, dropped = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = L.mkp_bedmethyl_merge_main(len(args), arr, ctypes.byref(written), ctypes.byref(dropped), err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    return int(written.value), int(dropped.value)


def dmr_pair(argv):
    """`modkit dmr pair` over regions (PairwiseDmr::run with -r, src/dmr/subcommands.rs) on the device: argv = ["-a", a.bed[.gz], "-b", b.bed[.gz],
    "-r", regions.bed, "--ref", ref.fa, "--base", "C", "-o", out.bed, "-f", "--header", "--min-valid-coverage", N, "--assign-code", "x:C", "--mask",
    "--missing", "quiet|warn|fail"]; the tables are read by the device reader (Context.dmr_add_file; MKP_HOST_BEDMETHYL=1: by the host reader).
    Single-site mode (no -r), --segment and more than one -a / -b are refused.  Returns the number of regions written."""
    L = lib()
    args = [str(a).encode() for a in argv]
    arr = (ctypes.c_char_p * max(1, len(args)))(*args)
    err = ctypes.create_string_buffer(2048)
    written = ctypes.c_uint64(0)
    rc = L.mkp_dmr_pair_main(len(args), arr, ctypes.byref(written), err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    return int(written.value)


def dmr_sites(argv):
    """`modkit dmr pair` without -r (SingleSiteDmrAnalysis::run, src/dmr/single_site.rs) on the device: argv = ["-a", a.bed[.gz], "-b", b.bed[.gz],
    "--ref", ref.fa, "--base", "C", "-o", out.bed, "-f", "--header", "--min-valid-coverage", N, "--assign-code", "x:C", "--mask", "--prior", A, B,
    "--delta", D, "--max-coverages", A, B, "-N", N, "--cap-coverages", "-i", BP, "--batch-size", N, "-t", T]; the tables are read by the device
    reader (Context.dmr_sites_add_file; MKP_HOST_BEDMETHYL=1: by the host reader).  -r, --segment and more than one -a / -b (that is
    dmr_replicates) are refused.
    Returns the number of sites written."""
    L = lib()
    args = [str(a).encode() for a in argv]
    arr = (ctypes.c_char_p * max(1, len(args)))(*args)
    err = ctypes.create_string_buffer(2048)
    written = ctypes.c_uint64(0)
    rc = L.mkp_dmr_sites_main(len(args), arr, ctypes.byref(written), err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    return int(written.value)


def dmr_replicates(argv):
    """`modkit dmr pair` without -r over replicates (SingleSiteDmrScore::new_multi, src/dmr/single_site.rs) on the device: argv = ["-a", a1.bed[.gz],
    "-a", a2.bed[.gz], .., "-b", b1.bed[.gz], "-b", b2.bed[.gz], .., "--ref", ref.fa, "--base", "C", ..] with every other flag of dmr_sites; at most
    16 tables a side.  With several tables on a side the rows gain balanced_map_pvalue, balanced_effect_size, pct_a_samples and pct_b_samples,
    with as many -a as -b (more than one) also replicate_map_pvalues and replicate_effect_sizes.  -r and --segment are refused.  Returns the
    number of sites written."""
    L = lib()
    args = [str(a).encode() for a in argv]
    arr = (ctypes.c_char_p * max(1, len(args)))(*args)
    err = ctypes.create_string_buffer(2048)
    written = ctypes.c_uint64(0)
    rc = L.mkp_dmr_reps_main(len(args), arr, ctypes.byref(written), err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    return int(written.value)


def extract_calls(argv):
    """`modkit extract calls` (EntryExtractCalls::run, src/extract/subcommand.rs:452): argv = [in_bam, out_tsv, flags...]."""
    L = lib()
    args = [str(a).encode() for a in argv]
    arr = (ctypes.c_char_p * len(args))(*args)
    err = ctypes.create_string_buffer(2048)
    rc = L.mkp_extract_calls_main(len(args), arr, err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    return rc


# ---------------------------------------------------------------------------------------------
# ctypes mirror of include/mkpileup.h for callers that drive shards directly (bench.py, tests)
class Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("tile_positions", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 6)]


class ModThreshold(ctypes.Structure):
    _fields_ = [("code_repr", ctypes.c_uint32), ("threshold", ctypes.c_float)]


class Caller(ctypes.Structure):
    _fields_ = [("default_threshold", ctypes.c_float), ("per_base_threshold", ctypes.c_float * 4), ("has_per_base", ctypes.c_uint8 * 4),
                ("per_mod", ctypes.POINTER(ModThreshold)), ("n_per_mod", ctypes.c_uint32), ("numeric_mode", ctypes.c_uint32),
                ("collapse_code", ctypes.c_uint32), ("edge_filter", ctypes.c_uint32), ("edge_start", ctypes.c_uint32),
                ("edge_end", ctypes.c_uint32), ("edge_inverted", ctypes.c_uint32), ("force_allow_implicit", ctypes.c_uint32),
                ("combine_strands", ctypes.c_uint32), ("max_depth", ctypes.c_uint32)]


class Shard(ctypes.Structure):
    _fields_ = [("tid", ctypes.c_int32), ("start", ctypes.c_uint32), ("end", ctypes.c_uint32), ("focus", ctypes.c_void_p),
                ("combos", ctypes.c_void_p), ("n_combos", ctypes.c_uint32)]


class Rows(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint64), ("pos", ctypes.POINTER(ctypes.c_uint32)), ("strand", ctypes.POINTER(ctypes.c_uint8)),
                ("code_repr", ctypes.POINTER(ctypes.c_uint32)), ("motif_idx", ctypes.POINTER(ctypes.c_int32)),
                ("n_valid", ctypes.POINTER(ctypes.c_uint32)), ("n_mod", ctypes.POINTER(ctypes.c_uint32)),
                ("n_canonical", ctypes.POINTER(ctypes.c_uint32)), ("n_other", ctypes.POINTER(ctypes.c_uint32)),
                ("n_delete", ctypes.POINTER(ctypes.c_uint32)), ("n_fail", ctypes.POINTER(ctypes.c_uint32)),
                ("n_diff", ctypes.POINTER(ctypes.c_uint32)), ("n_nocall", ctypes.POINTER(ctypes.c_uint32)),
                ("processed_records", ctypes.c_uint64), ("skipped_records", ctypes.c_uint64),
                ("partition_key", ctypes.POINTER(ctypes.c_uint32)), ("n_partition_keys", ctypes.c_uint32),
                ("partition_key_names", ctypes.POINTER(ctypes.c_char_p))]


class Region(ctypes.Structure):
    """mkp_region: one line of a regions BED (GenomeRegion, src/util.rs:850-857); strand_rule 1 '+', 2 '-', 3 both."""
    _fields_ = [("tid", ctypes.c_int32), ("start", ctypes.c_uint32), ("end", ctypes.c_uint32), ("strand_rule", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3)]


class StatsOut(ctypes.Structure):
    """mkp_stats_out: the per-region, per-code totals of `modkit stats`."""
    _fields_ = [("n_regions", ctypes.c_uint32), ("n_codes", ctypes.c_uint32), ("code_repr", ctypes.POINTER(ctypes.c_uint32)),
                ("n_mod", ctypes.POINTER(ctypes.c_uint64)), ("n_valid", ctypes.POINTER(ctypes.c_uint64)), ("contig_has_rows", ctypes.POINTER(ctypes.c_uint8))]


class DmrOut(ctypes.Structure):
    """mkp_dmr_out: per sample (a, b) and region the sums of `modkit dmr pair`, the scores and why a region is not written."""
    _fields_ = [("n_regions", ctypes.c_uint32), ("n_codes", ctypes.c_uint32), ("code_repr", ctypes.POINTER(ctypes.c_uint32)),
                ("n_mod", ctypes.POINTER(ctypes.c_uint64) * 2), ("has_code", ctypes.POINTER(ctypes.c_uint8) * 2),
                ("total", ctypes.POINTER(ctypes.c_uint64) * 2), ("n_rows", ctypes.POINTER(ctypes.c_uint64) * 2),
                ("bad", ctypes.POINTER(ctypes.c_uint8) * 2), ("contig_has_rows", ctypes.POINTER(ctypes.c_uint8) * 2),
                ("has_reference", ctypes.POINTER(ctypes.c_uint8)), ("score", ctypes.POINTER(ctypes.c_double)), ("state", ctypes.POINTER(ctypes.c_uint8))]


class DmrSitesConfig(ctypes.Structure):
    """mkp_dmr_sites_config"""
    _fields_ = [("contig_names", ctypes.POINTER(ctypes.c_char_p)), ("n_contigs", ctypes.c_uint32), ("bases", ctypes.c_char_p), ("n_bases", ctypes.c_uint32),
                ("codes", ctypes.POINTER(ctypes.c_uint32)), ("code_bases", ctypes.POINTER(ctypes.c_uint8)), ("n_lookup", ctypes.c_uint32),
                ("respect_mask", ctypes.c_uint32), ("min_valid_coverage", ctypes.c_uint64), ("prior_alpha", ctypes.c_double),
                ("prior_beta", ctypes.c_double), ("delta", ctypes.c_double), ("have_max_coverages", ctypes.c_uint32),
                ("max_coverages", ctypes.c_uint32 * 2), ("reserved", ctypes.c_uint32), ("n_sample_records", ctypes.c_uint64),
                ("interval_size", ctypes.c_uint64), ("batch_size", ctypes.c_uint64)]


class DmrSitesOut(ctypes.Structure):
    """mkp_dmr_sites_out: the written sites of `modkit dmr pair` without -r and the session's counters."""
    _fields_ = [("n_sites", ctypes.c_uint64), ("n_codes", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("code_repr", ctypes.POINTER(ctypes.c_uint32)),
                ("tid", ctypes.POINTER(ctypes.c_int32)), ("pos", ctypes.POINTER(ctypes.c_uint32)), ("strand", ctypes.POINTER(ctypes.c_uint8)),
                ("total", ctypes.POINTER(ctypes.c_uint32) * 2), ("n_mod", ctypes.POINTER(ctypes.c_uint32) * 2),
                ("has_code", ctypes.POINTER(ctypes.c_uint32) * 2), ("score", ctypes.POINTER(ctypes.c_double)),
                ("map_pvalue", ctypes.POINTER(ctypes.c_double)), ("effect_size", ctypes.POINTER(ctypes.c_double)),
                ("max_coverages", ctypes.c_uint32 * 2), ("n_sampled", ctypes.c_uint64 * 2), ("n_batches", ctypes.c_uint64),
                ("n_batches_dropped", ctypes.c_uint64), ("n_model_failures", ctypes.c_uint64)]


class DmrRepsOut(ctypes.Structure):
    """mkp_dmr_reps_out: mkp_dmr_sites_out over the collapsed counts, then what replicates add."""
    _fields_ = [("sites", DmrSitesOut), ("n_a", ctypes.c_uint32), ("n_b", ctypes.c_uint32), ("balanced_map_pvalue", ctypes.POINTER(ctypes.c_double)),
                ("balanced_effect_size", ctypes.POINTER(ctypes.c_double)), ("pct_samples", ctypes.POINTER(ctypes.c_uint32) * 2),
                ("n_rep", ctypes.POINTER(ctypes.c_uint32)), ("rep_pvalue", ctypes.POINTER(ctypes.c_double)),
                ("rep_effect", ctypes.POINTER(ctypes.c_double))]


class DmrSitesBatch(ctypes.Structure):
    """mkp_dmr_sites_batch: where a batch of the reference's walk begins inside a contig."""
    _fields_ = [("contig", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("start", ctypes.c_uint64), ("batch", ctypes.c_uint64)]


def host_dmr_site_score(a_mod, a_has, a_total, b_mod, b_has, b_total, prior=(0.55, 0.55), delta=0.05, max_coverages=(300, 300)):
    """mkp_host_dmr_site_score: one site's arithmetic as the kernel does it; a_mod / b_mod = counts per code column (ascending code), a_has /
    b_has = masks of the columns in the key set.  Returns ({"score", "ln_effect", "ln_null", "map_pvalue", "effect_size"}, failed)."""
    n = len(a_mod)
    am, bm = (ctypes.c_uint64 * max(1, n))(*a_mod), (ctypes.c_uint64 * max(1, n))(*b_mod)
    mc, vals, failed = (ctypes.c_uint32 * 2)(*max_coverages), (ctypes.c_double * 5)(), ctypes.c_int(0)
    rc = lib().mkp_host_dmr_site_score(am, int(a_has), int(a_total), bm, int(b_has), int(b_total), n, prior[0], prior[1], delta, mc, vals, ctypes.byref(failed))
    if rc != MKP_OK:
        raise MkpError(rc, "mkp_host_dmr_site_score failed")
    return dict(zip(("score", "ln_effect", "ln_null", "map_pvalue", "effect_size"), list(vals))), bool(failed.value)


def host_dmr_sites_batches(contig_lens, window_counts, interval_size):
    """mkp_host_dmr_sites_batches: the batch planner alone; window_counts = per contig the listed positions per window.  Returns
    ([(contig, start, batch)], number of batches)."""
    flat = [x for w in window_counts for x in w]
    lens = (ctypes.c_uint64 * max(1, len(contig_lens)))(*contig_lens)
    cnt = (ctypes.c_uint32 * max(1, len(flat)))(*flat)
    ent, nb = (DmrSitesBatch * max(1, len(flat)))(), ctypes.c_uint64(0)
    n = lib().mkp_host_dmr_sites_batches(lens, cnt, len(contig_lens), int(interval_size), ent, len(flat), ctypes.byref(nb))
    if n < 0:
        raise MkpError(int(n), "mkp_host_dmr_sites_batches failed")
    return [(int(ent[k].contig), int(ent[k].start), int(ent[k].batch)) for k in range(n)], int(nb.value)


def host_dmr_sites_gauss_legendre():
    """mkp_host_dmr_sites_gauss_legendre: (nodes, weights) of the 16-point rule on [-1, 1], nodes ascending."""
    x, w = (ctypes.c_double * 16)(), (ctypes.c_double * 16)()
    lib().mkp_host_dmr_sites_gauss_legendre(x, w)
    return list(x), list(w)


def dmr_sites_out_from(d):
    """A DmrSitesOut over numpy copies of the dict Context.dmr_sites_get returns; returns (struct, arrays to keep alive)."""
    import numpy as np
    u32p, f64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    keep = {"codes": np.ascontiguousarray(np.asarray(d["codes"], dtype=np.uint32)), "tid": np.ascontiguousarray(np.asarray(d["tid"], dtype=np.int32)),
            "pos": np.ascontiguousarray(np.asarray(d["pos"], dtype=np.uint32)),
            "strand": np.ascontiguousarray(np.asarray([ord(c) if isinstance(c, str) else int(c) for c in d["strand"]], dtype=np.uint8))}
    o = DmrSitesOut(n_sites=len(keep["pos"]), n_codes=len(keep["codes"]), code_repr=keep["codes"].ctypes.data_as(u32p),
                    tid=keep["tid"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), pos=keep["pos"].ctypes.data_as(u32p),
                    strand=keep["strand"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    for f in ("total", "n_mod", "has_code"):
        for s in range(2):
            a = keep[f, s] = np.ascontiguousarray(np.asarray(d[f][s], dtype=np.uint32))
            getattr(o, f)[s] = a.ctypes.data_as(u32p)
    for f in ("score", "map_pvalue", "effect_size"):
        keep[f] = np.ascontiguousarray(np.asarray(d[f], dtype=np.float64))
        setattr(o, f, keep[f].ctypes.data_as(f64p))
    return o, keep


def write_dmr_sites_table(sites, contig_names, out_path, header=False):
    """mkp_host_dmr_sites_table: the 16-column table of `sites` (the dict Context.dmr_sites_get returns, or one a caller filled)."""
    o, keep = dmr_sites_out_from(sites)
    enc = [str(n).encode() for n in contig_names]
    arr = (ctypes.c_char_p * max(1, len(enc)))(*enc)
    rc = lib().mkp_host_dmr_sites_table(ctypes.byref(o), arr, len(enc), int(bool(header)), str(out_path).encode())
    del keep
    if rc != MKP_OK:
        raise MkpError(rc, "mkp_host_dmr_sites_table failed")


def host_dmr_reps_balance(n_mod, has_code, total):
    """mkp_host_dmr_reps_balance: collapse_counts(_, true) of one side of one site.  n_mod[s] = sample s's counts per code column, has_code[s] the
    mask of the columns in its key set, total[s] its total.  Returns (counts per column, column mask, total, failed)."""
    n, k = len(total), (len(n_mod[0]) if n_mod else 0)
    flat = [int(x) for row in n_mod for x in row]
    nm, hs, tt = (ctypes.c_uint64 * max(1, len(flat)))(*flat), (ctypes.c_uint32 * max(1, n))(*has_code), (ctypes.c_uint64 * max(1, n))(*total)
    om, oh, ot, failed = (ctypes.c_uint64 * max(1, k))(), ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_int(0)
    rc = lib().mkp_host_dmr_reps_balance(nm, hs, tt, n, k, om, ctypes.byref(oh), ctypes.byref(ot), ctypes.byref(failed))
    if rc != MKP_OK:
        raise MkpError(rc, "mkp_host_dmr_reps_balance failed")
    return list(om)[:k], int(oh.value), int(ot.value), bool(failed.value)


def host_dmr_reps_pct(n_present, n_samples):
    """mkp_host_dmr_reps_pct: floor(n_present / n_samples * 100) in f32, the pct_a_samples / pct_b_samples of a site."""
    return int(lib().mkp_host_dmr_reps_pct(int(n_present), int(n_samples)))


def write_dmr_reps_table(sites, contig_names, out_path, header=False):
    """mkp_host_dmr_reps_table: the table of `sites` (the dict Context.dmr_reps_get returns, or one a caller filled: the keys of
    write_dmr_sites_table's, "n_a", "n_b", "balanced_map_pvalue", "balanced_effect_size", "pct_samples" (a, b), "n_rep" and, with matched sides,
    "rep_pvalue" / "rep_effect" of shape [n, n_a])."""
    import numpy as np
    u32p, f64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    inner, keep = dmr_sites_out_from(sites)
    o = DmrRepsOut(sites=inner, n_a=int(sites["n_a"]), n_b=int(sites["n_b"]))
    n = len(keep["pos"])
    for f in ("balanced_map_pvalue", "balanced_effect_size"):
        keep[f] = np.ascontiguousarray(np.asarray(sites[f], dtype=np.float64))
        setattr(o, f, keep[f].ctypes.data_as(f64p))
    for s in range(2):
        a = keep["pct", s] = np.ascontiguousarray(np.asarray(sites["pct_samples"][s], dtype=np.uint32))
        o.pct_samples[s] = a.ctypes.data_as(u32p)
    keep["n_rep"] = np.ascontiguousarray(np.asarray(sites["n_rep"], dtype=np.uint32))
    o.n_rep = keep["n_rep"].ctypes.data_as(u32p)
    if o.n_a == o.n_b and o.n_a > 1:
        for f in ("rep_pvalue", "rep_effect"):
            keep[f] = np.ascontiguousarray(np.asarray(sites[f], dtype=np.float64).reshape(n, o.n_a))
            setattr(o, f, keep[f].ctypes.data_as(f64p))
    enc = [str(x).encode() for x in contig_names]
    arr = (ctypes.c_char_p * max(1, len(enc)))(*enc)
    rc = lib().mkp_host_dmr_reps_table(ctypes.byref(o), arr, len(enc), int(bool(header)), str(out_path).encode())
    del keep
    if rc != MKP_OK:
        raise MkpError(rc, "mkp_host_dmr_reps_table failed")


DMR_WRITTEN, DMR_NO_CONTIG, DMR_NO_REFERENCE, DMR_BAD, DMR_MODEL = 0, 1, 2, 3, 4   # MKP_DMR_* (mkp_dmr_out.state)
STRAND_RULES = {"+": 1, "-": 2, ".": 3}


def code_repr(code):
    """ModCodeRepr as the library's u32: a one-character code's code point, or a ChEBI number | 1 << 31 (ModCodeRepr::parse)."""
    if isinstance(code, str):
        return ord(code) if len(code) == 1 else (int(code) | (1 << 31))
    return int(code)


class RegionSet:
    """A parsed regions BED (mkp_host_parse_regions): `regions` = [(chrom, start, end, name or ".", strand "+-."), ...], tids by `contig_names`."""

    def __init__(self, bed_path, contig_names, localize=False, dmr=False):
        """localize=True: the tolerant loader of `modkit localize` (mkp_host_parse_localize_regions); `skipped` = the lines that failed to parse.
        dmr=True: the loader of `modkit dmr pair` (mkp_host_parse_dmr_regions: leading '#' lines skipped)."""
        self.L = lib()
        names = [str(n).encode() for n in contig_names]
        arr = (ctypes.c_char_p * max(1, len(names)))(*names)
        self.h = ctypes.c_void_p()
        self.skipped = 0
        err = ctypes.create_string_buffer(2048)
        if localize:
            skipped = ctypes.c_uint32(0)
            rc = self.L.mkp_host_parse_localize_regions(str(bed_path).encode(), arr, len(names), ctypes.byref(self.h), ctypes.byref(skipped), err, len(err))
            self.skipped = int(skipped.value)
        else:
            parse = self.L.mkp_host_parse_dmr_regions if dmr else self.L.mkp_host_parse_regions
            rc = parse(str(bed_path).encode(), arr, len(names), ctypes.byref(self.h), err, len(err))
        if rc != MKP_OK:
            raise MkpError(rc, err.value.decode(errors="replace"))
        self.n = self.L.mkp_region_set_size(self.h)
        self.array = self.L.mkp_region_set_regions(self.h)

    @property
    def regions(self):
        return [(self.L.mkp_region_set_chrom(self.h, i).decode(), int(self.array[i].start), int(self.array[i].end),
                 self.L.mkp_region_set_name(self.h, i).decode(), "?+-."[self.array[i].strand_rule]) for i in range(self.n)]

    @property
    def tids(self):
        return [int(self.array[i].tid) for i in range(self.n)]

    def write_table(self, counts, out_path, header=True):
        """The `modkit stats` table of `counts` (a StatsOut, or the dict Context.stats_get returns) for these regions (mkp_host_stats_table)."""
        keep = None
        if isinstance(counts, dict):
            counts, keep = stats_out_from(counts)
        rc = self.L.mkp_host_stats_table(self.h, ctypes.byref(counts), int(bool(header)), str(out_path).encode())
        del keep
        if rc != MKP_OK:
            raise MkpError(rc, "mkp_host_stats_table failed")

    def write_dmr_table(self, counts, out_path, header=False):
        """The `modkit dmr pair` table of `counts` (the dict Context.dmr_get returns, or one a caller filled: "score" / "state" may be left out
        and are then worked out by mkp_host_dmr_judge) for these regions (mkp_host_dmr_table)."""
        o, keep = dmr_out_from(counts)
        rc = self.L.mkp_host_dmr_table(self.h, ctypes.byref(o), int(bool(header)), str(out_path).encode())
        del keep
        if rc != MKP_OK:
            raise MkpError(rc, "mkp_host_dmr_table failed")

    def close(self):
        if self.h:
            self.L.mkp_region_set_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stats_out_from(d):
    """A StatsOut over numpy copies of {"codes", "n_mod", "n_valid", "contig_has_rows"}; returns (struct, arrays to keep alive)."""
    import numpy as np
    codes = np.ascontiguousarray(np.asarray(d["codes"], dtype=np.uint32))
    n_mod = np.ascontiguousarray(np.asarray(d["n_mod"], dtype=np.uint64))
    n_valid = np.ascontiguousarray(np.asarray(d["n_valid"], dtype=np.uint64))
    has = np.ascontiguousarray(np.asarray(d["contig_has_rows"], dtype=np.uint8))
    o = StatsOut(n_regions=len(has), n_codes=len(codes), code_repr=codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                 n_mod=n_mod.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n_valid=n_valid.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                 contig_has_rows=has.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return o, (codes, n_mod, n_valid, has)


def dmr_out_from(d):
    """A DmrOut over numpy copies of the dict Context.dmr_get returns; without "score" / "state" they come from mkp_host_dmr_judge.  Returns
    (struct, arrays to keep alive)."""
    import numpy as np
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    keep = {"codes": np.ascontiguousarray(np.asarray(d["codes"], dtype=np.uint32))}
    n, k = len(d["has_reference"]), len(keep["codes"])
    o = DmrOut(n_regions=n, n_codes=k, code_repr=keep["codes"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    for f, dt, pt in (("n_mod", np.uint64, u64p), ("has_code", np.uint8, u8p), ("total", np.uint64, u64p), ("n_rows", np.uint64, u64p),
                      ("bad", np.uint8, u8p), ("contig_has_rows", np.uint8, u8p)):
        for s in range(2):
            a = keep[f, s] = np.ascontiguousarray(np.asarray(d[f][s], dtype=dt))
            getattr(o, f)[s] = a.ctypes.data_as(pt)
    keep["ref"] = np.ascontiguousarray(np.asarray(d["has_reference"], dtype=np.uint8))
    o.has_reference = keep["ref"].ctypes.data_as(u8p)
    if "score" in d and "state" in d:
        keep["score"] = np.ascontiguousarray(np.asarray(d["score"], dtype=np.float64))
        keep["state"] = np.ascontiguousarray(np.asarray(d["state"], dtype=np.uint8))
    else:
        keep["score"], keep["state"] = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint8)
        rc = lib().mkp_host_dmr_judge(ctypes.byref(o), keep["score"].ctypes.data_as(ctypes.POINTER(ctypes.c_double)), keep["state"].ctypes.data_as(u8p))
        if rc != MKP_OK:
            raise MkpError(rc, "mkp_host_dmr_judge failed")
    o.score, o.state = keep["score"].ctypes.data_as(ctypes.POINTER(ctypes.c_double)), keep["state"].ctypes.data_as(u8p)
    return o, keep


def dmr_default_lookup():
    """MOD_CODE_TO_DNA_BASE as {code_repr: base letter} (mkp_dmr_default_lookup)."""
    L = lib()
    n = L.mkp_dmr_default_lookup(None, None, 0)
    codes, bases = (ctypes.c_uint32 * n)(), (ctypes.c_uint8 * n)()
    L.mkp_dmr_default_lookup(codes, bases, n)
    return {int(codes[k]): "ACGT"[bases[k]] for k in range(n)}


class LocalizeOut(ctypes.Structure):
    """mkp_localize_out: the per-code, per-offset totals of `modkit localize`; arrays [code * (2 window + 1) + offset + window]."""
    _fields_ = [("n_codes", ctypes.c_uint32), ("window", ctypes.c_uint32), ("code_repr", ctypes.POINTER(ctypes.c_uint32)),
                ("n_mod", ctypes.POINTER(ctypes.c_uint64)), ("n_valid", ctypes.POINTER(ctypes.c_uint64)), ("n_rows", ctypes.POINTER(ctypes.c_uint64))]


STRANDED = {None: 0, "same": 1, "opposite": 2}
STRANDED_FEATURES = {None: 0, "+": 1, "-": 2, ".": 3}


def localize_tile_offsets():
    """mkp_localize_tile_offsets: the offsets one workgroup of the localize kernel owns."""
    return int(lib().mkp_localize_tile_offsets())


def merge_tile_rows():
    """mkp_merge_tile_rows: the rows between two tile cuts of the merge kernel."""
    return int(lib().mkp_merge_tile_rows())


def _bedmethyl_file_runs(L, h):
    """the runs of a mkp_bedmethyl_file handle as [(chrom, rows dict), ...]; frees the handle"""
    try:
        out = []
        for k in range(L.mkp_bedmethyl_file_runs(h)):
            r = Rows()
            if L.mkp_bedmethyl_file_rows(h, k, ctypes.byref(r)) != MKP_OK:
                raise MkpError(-1, "mkp_bedmethyl_file_rows failed")
            out.append((L.mkp_bedmethyl_file_chrom(h, k).decode(), rows_to_numpy(r)))
        return out
    finally:
        L.mkp_bedmethyl_file_free(h)


def read_bedmethyl_runs(path):
    """mkp_host_read_bedmethyl: a bedMethyl file, plain text or bgzip compressed (inflated by the host's own decoder, every block's CRC-32
    checked; tabs and / or blanks, '#' lines skipped, the code = the name up to its first comma, n_valid = the score column) as
    [(chrom, rows dict with all eleven columns), ...], one entry per run of lines on one contig, file order.  No device is used:
    Context.read_bedmethyl_runs reads the same files on the GPU."""
    L = lib()
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(2048)
    rc = L.mkp_host_read_bedmethyl(str(path).encode(), ctypes.byref(h), err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    return _bedmethyl_file_runs(L, h)


def bedmethyl_chunk_bytes():
    """mkp_bedmethyl_chunk_bytes: the bytes of text a workgroup of the device bedMethyl reader's line kernels takes."""
    return int(lib().mkp_bedmethyl_chunk_bytes())


def genome_sizes(path):
    """mkp_host_parse_genome_sizes: [(contig, length), ...] of a `chrom<whitespace>length` file; a later line for a contig replaces its length."""
    L = lib()
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(2048)
    rc = L.mkp_host_parse_genome_sizes(str(path).encode(), ctypes.byref(h), err, len(err))
    if rc != MKP_OK:
        raise MkpError(rc, err.value.decode(errors="replace"))
    try:
        return [(L.mkp_genome_sizes_name(h, i).decode(), int(L.mkp_genome_sizes_length(h, i))) for i in range(L.mkp_genome_sizes_size(h))]
    finally:
        L.mkp_genome_sizes_free(h)


def write_localize_table(counts, out_path):
    """mkp_host_localize_table: the `modkit localize` table of the dict Context.localize_get returns."""
    import numpy as np
    codes = np.ascontiguousarray(np.asarray(counts["codes"], dtype=np.uint32))
    cols = [np.ascontiguousarray(np.asarray(counts[f], dtype=np.uint64)) for f in ("n_mod", "n_valid", "n_rows")]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    o = LocalizeOut(n_codes=len(codes), window=int(counts["window"]), code_repr=codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                    n_mod=cols[0].ctypes.data_as(u64p), n_valid=cols[1].ctypes.data_as(u64p), n_rows=cols[2].ctypes.data_as(u64p))
    rc = lib().mkp_host_localize_table(ctypes.byref(o), str(out_path).encode())
    if rc != MKP_OK:
        raise MkpError(rc, "mkp_host_localize_table failed")


class HemiRows(ctypes.Structure):
    """mkp_hemi_rows: duplex pattern counts (DuplexPatternCounts, src/pileup/duplex.rs:32-56)."""
    _u32p = ctypes.POINTER(ctypes.c_uint32)
    _fields_ = [("n_rows", ctypes.c_uint64), ("pos", _u32p), ("primary_base", ctypes.POINTER(ctypes.c_uint8)), ("pattern_pos", _u32p),
                ("pattern_neg", _u32p), ("n_valid", _u32p), ("count", _u32p), ("n_canonical", _u32p), ("n_other_pattern", _u32p),
                ("n_delete", _u32p), ("n_fail", _u32p), ("n_diff", _u32p), ("n_nocall", _u32p),
                ("processed_records", ctypes.c_uint64), ("skipped_records", ctypes.c_uint64)]


HEMI_ROW_FIELDS = ("pos", "primary_base", "pattern_pos", "pattern_neg", "n_valid", "count", "n_canonical", "n_other_pattern", "n_delete",
                   "n_fail", "n_diff", "n_nocall")


class SummaryOut(ctypes.Structure):
    """mkp_summary_out: ModSummary (src/summarize.rs:21-46) as counts."""
    _fields_ = [("total_reads_used", ctypes.c_uint64), ("reads_with_mod_calls", ctypes.c_uint64 * 4), ("threshold", ctypes.c_float * 4),
                ("has_threshold", ctypes.c_uint8 * 4), ("n_rows", ctypes.c_uint32), ("base", ctypes.POINTER(ctypes.c_uint8)),
                ("code_repr", ctypes.POINTER(ctypes.c_uint32)), ("pass_count", ctypes.POINTER(ctypes.c_uint64)), ("fail_count", ctypes.POINTER(ctypes.c_uint64))]


class Stats(ctypes.Structure):
    _fields_ = [("pack_ms", ctypes.c_double), ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double),
                ("decode_kernel_ms", ctypes.c_double), ("pileup_kernel_ms", ctypes.c_double), ("gather_kernel_ms", ctypes.c_double),
                ("n_reads", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("n_rows", ctypes.c_uint64), ("n_tiles", ctypes.c_uint64),
                ("n_positions", ctypes.c_uint64), ("alg_bytes_decode", ctypes.c_uint64), ("alg_bytes_pileup", ctypes.c_uint64),
                ("rows_kernel_ms", ctypes.c_double), ("alg_bytes_rows", ctypes.c_uint64),
                ("stream_bytes", ctypes.c_uint64), ("alg_bytes_agg_survey", ctypes.c_uint64), ("slot_pipeline", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class RunReport(ctypes.Structure):
    _fields_ = [("load_ms", ctypes.c_double), ("threshold_ms", ctypes.c_double), ("focus_ms", ctypes.c_double), ("pack_ms", ctypes.c_double),
                ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double), ("write_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double), ("n_rows", ctypes.c_uint64), ("n_positions", ctypes.c_uint64), ("n_shards", ctypes.c_uint64),
                ("processed_records", ctypes.c_uint64), ("skipped_records", ctypes.c_uint64), ("threshold", ctypes.c_float * 4),
                ("has_threshold", ctypes.c_uint8 * 4),
                ("grid_wait_ms", ctypes.c_double), ("callback_ms", ctypes.c_double), ("ingest_kernel_ms", ctypes.c_double), ("ingest_upload_ms", ctypes.c_double),
                ("ingest_table_ms", ctypes.c_double), ("ingest_pack_ms", ctypes.c_double), ("ingest_comp_bytes", ctypes.c_uint64), ("ingest_raw_bytes", ctypes.c_uint64),
                ("ingest_blocks", ctypes.c_uint64), ("ingest_records", ctypes.c_uint64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("threshold", "has_threshold")}
        d["thresholds"] = {"ACGT"[i]: float(self.threshold[i]) for i in range(4) if self.has_threshold[i]}
        return d


def _region_array(regions):
    """(Region array, n) of a RegionSet, or of [(tid, start, end, strand "+-." or rule 1..3), ...]."""
    if isinstance(regions, RegionSet):
        return regions.array, regions.n
    n = len(regions)
    arr = (Region * max(1, n))()
    for i, (tid, start, end, rule) in enumerate(regions):
        arr[i].tid, arr[i].start, arr[i].end = int(tid), int(start), int(end)
        arr[i].strand_rule = STRAND_RULES[rule] if isinstance(rule, str) else int(rule)
    return arr, n


MERGE_COUNT_FIELDS = ("n_valid", "n_mod", "n_canonical", "n_other", "n_delete", "n_fail", "n_diff", "n_nocall")


def _rows_struct(rows, all_columns=False):
    """(Rows over the five columns the row reducers read — or all eleven, for the merge —, the arrays it points into) of a dict of arrays."""
    import numpy as np
    cols = {f: np.ascontiguousarray(np.asarray(rows[f], dtype=np.uint8 if f == "strand" else np.uint32))
            for f in ("pos", "strand", "code_repr") + (MERGE_COUNT_FIELDS if all_columns else ("n_valid", "n_mod"))}
    r = Rows()
    r.n_rows = len(cols["pos"])
    for f, a in cols.items():
        setattr(r, f, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8 if f == "strand" else ctypes.c_uint32)))
    return r, cols


def _copy_out(p, shape, dt):
    """A copy of the library's array behind p; an empty shape has no pointer to read."""
    import numpy as np
    return np.ctypeslib.as_array(p, shape=shape).copy() if all(shape) else np.zeros(shape, dtype=dt)


class Context:
    """One mkp_ctx (one per host thread; binds to one GPU)."""

    def __init__(self, device=0, tile_positions=0):
        self.L = lib()
        self.h = ctypes.c_void_p()
        cfg = Config(device=device, tile_positions=tile_positions)
        rc = self.L.mkp_ctx_create(ctypes.byref(cfg), ctypes.byref(self.h))
        if rc != MKP_OK:
            raise MkpError(rc, "mkp_ctx_create failed (no gfx950 device visible?)")

    def _check(self, rc):
        if rc != MKP_OK:
            raise MkpError(rc, self.L.mkp_last_error(self.h).decode(errors="replace"))

    def close(self):
        if self.h:
            self.L.mkp_ctx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def set_caller(self, default_threshold=0.0, per_base=None, per_mod=None, numeric_mode=0, collapse_code=0, combine_strands=False,
                   force_allow_implicit=False, edge=None, max_depth=8000):
        c = Caller()
        c.default_threshold = default_threshold
        for b, t in (per_base or {}).items():
            i = "ACGT".index(b) if isinstance(b, str) else int(b)
            c.per_base_threshold[i] = t
            c.has_per_base[i] = 1
        pm = list((per_mod or {}).items())
        arr = (ModThreshold * max(1, len(pm)))()
        for i, (code, t) in enumerate(pm):
            arr[i].code_repr = ord(code) if isinstance(code, str) else int(code)
            arr[i].threshold = t
        c.per_mod = arr
        c.n_per_mod = len(pm)
        c.numeric_mode, c.collapse_code, c.combine_strands = numeric_mode, collapse_code, int(combine_strands)
        c.force_allow_implicit, c.max_depth = int(force_allow_implicit), max_depth
        if edge:
            c.edge_filter, c.edge_start, c.edge_end, c.edge_inverted = 1, edge[0], edge[1], int(edge[2]) if len(edge) > 2 else 0
        self._check(self.L.mkp_set_caller(self.h, ctypes.byref(c)))

    def estimate_thresholds(self, bam, argv=()):
        args = [str(a).encode() for a in argv]
        arr = (ctypes.c_char_p * max(1, len(args)))(*args)
        thr = (ctypes.c_float * 4)()
        has = (ctypes.c_uint8 * 4)()
        self._check(self.L.mkp_estimate_thresholds(self.h, str(bam).encode(), len(args), arr, thr, has))
        return {"ACGT"[i]: float(thr[i]) for i in range(4) if has[i]}

    def histogram_begin(self):
        self._check(self.L.mkp_histogram_begin(self.h))

    def histogram_add_bam(self, bam, argv=()):
        """Sample this rank's windows of `bam` (argv: sampling flags, --gpus-rank/--gpus-world) into the HBM-resident sample."""
        args = [str(a).encode() for a in argv]
        arr = (ctypes.c_char_p * max(1, len(args)))(*args)
        self._check(self.L.mkp_histogram_add_bam(self.h, str(bam).encode(), len(args), arr))

    def histogram_allreduce(self, comm, base, level, prefix=0):
        """histogram_get summed over the ranks of an RCCL communicator (modkit_amd.distributed.RcclComm), in HBM over xGMI."""
        import numpy as np
        out = np.zeros(65536, dtype=np.uint64)
        i = "ACGT".index(base) if isinstance(base, str) else int(base)
        self._check(self.L.mkp_histogram_allreduce(self.h, comm.handle, i, level, prefix, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def histogram_get(self, base, level, prefix=0):
        """uint64[65536] numpy array: level 0 = top 16 bits of the f32 patterns of `base`'s sample, level 1 = low 16 bits under `prefix`."""
        import numpy as np
        out = np.zeros(65536, dtype=np.uint64)
        i = "ACGT".index(base) if isinstance(base, str) else int(base)
        self._check(self.L.mkp_histogram_get(self.h, i, level, prefix, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def process_region(self, bam, tid, start, end):
        sh = Shard(tid=tid, start=start, end=end, focus=None, combos=None, n_combos=0)
        rows = Rows()
        self._check(self.L.mkp_process_region(self.h, str(bam).encode(), ctypes.byref(sh), ctypes.byref(rows)))
        return rows

    def pileup_run(self, argv):
        """`modkit pileup` on this context (mkp_pileup_run): the last shard stays resident for rerun(); returns the stage report."""
        args = [str(a).encode() for a in argv]
        arr = (ctypes.c_char_p * len(args))(*args)
        rep = RunReport()
        self._check(self.L.mkp_pileup_run(self.h, len(args), arr, ctypes.byref(rep)))
        return rep

    def pileup_run_cb(self, argv, thresholds):
        """`modkit pileup` with the pass thresholds decided by the caller (mkp_pileup_run_cb — the multi-GPU form: argv carries --gpus-rank /
        --gpus-world and no threshold flags).  The library ingests this rank's shards ahead, then calls `thresholds(have_sample)` once:
        have_sample True (`-f 1.0`): this context's histograms hold the sample of this rank's shards — reduce them over the ranks and
        evaluate the percentile; False: nothing was sampled, supply the values.  It returns {base letter: f32}.  Returns the stage report."""
        args = [str(a).encode() for a in argv]
        arr = (ctypes.c_char_p * len(args))(*args)
        rep = RunReport()
        failure = []

        def _cb(user, ctx, have_sample, thr, has):
            try:
                got = thresholds(bool(have_sample))
                for i, b in enumerate("ACGT"):
                    if b in got:
                        thr[i] = float(got[b]); has[i] = 1
                    else:
                        thr[i] = 0.0; has[i] = 0
                return MKP_OK
            except BaseException as e:   # (must not unwind through the C frames)
                failure.append(e)
                return -2
        fn = THRESHOLD_FN(_cb)
        rc = self.L.mkp_pileup_run_cb(self.h, len(args), arr, fn, None, ctypes.byref(rep))
        if failure:
            raise failure[0]
        self._check(rc)
        return rep

    def pileup_hemi_run(self, argv):
        """`modkit pileup-hemi` on this context (mkp_pileup_hemi_run); returns the stage report."""
        args = [str(a).encode() for a in argv]
        arr = (ctypes.c_char_p * len(args))(*args)
        rep = RunReport()
        self._check(self.L.mkp_pileup_hemi_run(self.h, len(args), arr, ctypes.byref(rep)))
        return rep

    def hemi_shard_run(self, partner_offset, interval_starts=()):
        """mkp_hemi_shard_run on the shard begun with shard_begin / add_records; returns a dict of numpy arrays."""
        import numpy as np
        iv = (ctypes.c_uint32 * max(1, len(interval_starts)))(*[int(x) for x in interval_starts])
        rows = HemiRows()
        self._check(self.L.mkp_hemi_shard_run(self.h, int(partner_offset), iv if len(interval_starts) else None, len(interval_starts), ctypes.byref(rows)))
        n = int(rows.n_rows)
        out = {f: (np.ctypeslib.as_array(getattr(rows, f), shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint32)) for f in HEMI_ROW_FIELDS}
        out["processed_records"], out["skipped_records"] = int(rows.processed_records), int(rows.skipped_records)
        return out

    def sample_probs(self, bam, percentiles=(0.1, 0.5, 0.9), argv=()):
        """`modkit sample-probs` percentiles (mkp_sample_probs): {base: {"n": sampled calls, "percentiles": {q: value}}}; values are f32."""
        import numpy as np
        args = [str(a).encode() for a in argv]
        arr = (ctypes.c_char_p * max(1, len(args)))(*args)
        qs = np.asarray(percentiles, dtype=np.float32)
        vals = np.zeros((4, len(qs)), dtype=np.float32)
        has = (ctypes.c_uint8 * 4)()
        n = (ctypes.c_uint64 * 4)()
        f32p = ctypes.POINTER(ctypes.c_float)
        self._check(self.L.mkp_sample_probs(self.h, str(bam).encode(), len(args), arr, qs.ctypes.data_as(f32p), len(qs), vals.ctypes.data_as(f32p), has, n))
        return {"ACGT"[b]: {"n": int(n[b]), "percentiles": {float(qs[k]): vals[b, k] for k in range(len(qs))}} for b in range(4) if has[b]}

    def summary(self, bam, argv=()):
        """`modkit summary` as counts (mkp_summary): {"total", "reads_with": {base: n}, "threshold": {base: f32}, "rows": {(base, code): (pass, fail)}};
        code "-" = canonical, a letter, or a ChEBI number as text."""
        args = [str(a).encode() for a in argv]
        arr = (ctypes.c_char_p * max(1, len(args)))(*args)
        o = SummaryOut()
        self._check(self.L.mkp_summary(self.h, str(bam).encode(), len(args), arr, ctypes.byref(o)))
        def code(c):
            return "-" if c == 0 else str(c & 0x7fffffff) if c & 0x80000000 else chr(c)
        return {"total": int(o.total_reads_used), "reads_with": {"ACGT"[b]: int(o.reads_with_mod_calls[b]) for b in range(4) if o.reads_with_mod_calls[b]},
                "threshold": {"ACGT"[b]: float(o.threshold[b]) for b in range(4) if o.has_threshold[b]},
                "rows": {("ACGT"[o.base[i]], code(o.code_repr[i])): (int(o.pass_count[i]), int(o.fail_count[i])) for i in range(o.n_rows)}}

    def bgzf_inflate(self, data):
        """mkp_bgzf_inflate: inflate a BGZF file image (bytes) on the device; returns (inflated bytes, kernel ms)."""
        out, n, ms = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_double()
        self._check(self.L.mkp_bgzf_inflate(self.h, data, len(data), ctypes.byref(out), ctypes.byref(n), ctypes.byref(ms)))
        return ctypes.string_at(out, n.value) if n.value else b"", ms.value

    def set_partition_tags(self, tags):
        """mkp_set_partition_tags: two-character SAM tag names; an empty list clears."""
        enc = [str(t).encode() for t in tags]
        arr = (ctypes.c_char_p * max(1, len(enc)))(*enc)
        self._check(self.L.mkp_set_partition_tags(self.h, arr, len(enc)))

    def stats_begin(self, regions, codes=None, min_coverage=1):
        """mkp_stats_begin: regions = a RegionSet, or [(tid, start, end, strand "+-." or rule 1..3), ...]; codes = the `--mod-codes` list
        (letters, ChEBI numbers as text, or code_repr ints) or None for every code met; min_coverage = `--min-coverage`."""
        arr, n = _region_array(regions)
        cs = [code_repr(c) for c in (codes or [])]
        carr = (ctypes.c_uint32 * max(1, len(cs)))(*cs)
        self._check(self.L.mkp_stats_begin(self.h, arr, n, carr, len(cs), int(min_coverage)))

    def stats_add_resident(self):
        """mkp_stats_add_resident: add the rows the last shard run left in HBM to the region table."""
        self._check(self.L.mkp_stats_add_resident(self.h))

    def stats_add_rows(self, tid, rows):
        """mkp_stats_add_rows: rows of ONE contig, ascending pos, as a dict of arrays (pos, strand as bytes '+-.', code_repr, n_valid, n_mod:
        what read_bedmethyl / rows_to_numpy give); they are uploaded and reduced by the same kernels."""
        r, _keep = _rows_struct(rows)
        self._check(self.L.mkp_stats_add_rows(self.h, int(tid), ctypes.byref(r)))

    def stats_get(self):
        """mkp_stats_get: {"codes": u32[n_codes] sorted, "n_mod" / "n_valid": u64[n_regions, n_codes], "contig_has_rows": u8[n_regions]}."""
        o = StatsOut()
        self._check(self.L.mkp_stats_get(self.h, ctypes.byref(o)))
        n, k, arr = int(o.n_regions), int(o.n_codes), _copy_out
        return {"codes": arr(o.code_repr, (k,), "u4"), "n_mod": arr(o.n_mod, (n, k), "u8"), "n_valid": arr(o.n_valid, (n, k), "u8"),
                "contig_has_rows": arr(o.contig_has_rows, (n,), "u1")}

    def localize_begin(self, regions, contig_lengths, window=2000, stranded=None, stranded_features=None):
        """mkp_localize_begin: regions = a RegionSet, or [(tid, start, end, strand "+-." or rule 1..3), ...] (start > end allowed);
        contig_lengths[tid] = the genome-sizes table; stranded = None / "same" / "opposite"; stranded_features = None / "+" / "-" / "."."""
        arr, n = _region_array(regions)
        lens = (ctypes.c_uint64 * max(1, len(contig_lengths)))(*[int(x) for x in contig_lengths])
        self._check(self.L.mkp_localize_begin(self.h, arr, n, lens, len(contig_lengths), int(window), STRANDED[stranded], STRANDED_FEATURES[stranded_features]))

    def localize_add_resident(self):
        """mkp_localize_add_resident: add the rows the last shard run left in HBM to the offset table."""
        self._check(self.L.mkp_localize_add_resident(self.h))

    def localize_add_rows(self, tid, rows):
        """mkp_localize_add_rows: rows of ONE contig, ascending pos, as stats_add_rows takes them."""
        r, _keep = _rows_struct(rows)
        self._check(self.L.mkp_localize_add_rows(self.h, int(tid), ctypes.byref(r)))

    def localize_get(self):
        """mkp_localize_get: {"codes": u32[n_codes] sorted, "window": w, "n_mod" / "n_valid" / "n_rows": u64[n_codes, 2 w + 1]}, column
        offset + w; a (code, offset) cell is a table line when its n_rows is not 0."""
        o = LocalizeOut()
        self._check(self.L.mkp_localize_get(self.h, ctypes.byref(o)))
        k, n, arr = int(o.n_codes), 2 * int(o.window) + 1, _copy_out
        return {"codes": arr(o.code_repr, (k,), "u4"), "window": int(o.window), "n_mod": arr(o.n_mod, (k, n), "u8"),
                "n_valid": arr(o.n_valid, (k, n), "u8"), "n_rows": arr(o.n_rows, (k, n), "u8")}

    def merge_begin(self, contig_lengths):
        """mkp_merge_begin: contig_lengths[tid] = the genome-sizes table; drops the tables of the session before."""
        lens = (ctypes.c_uint64 * max(1, len(contig_lengths)))(*[int(x) for x in contig_lengths])
        self._check(self.L.mkp_merge_begin(self.h, lens, len(contig_lengths)))

    def merge_add_rows(self, tid, rows):
        """mkp_merge_add_rows: rows of ONE contig, ascending pos (any order inside a position), as a dict of arrays with all eleven columns
        (what read_bedmethyl / read_bedmethyl_runs / rows_to_numpy give); joined into the contig's table on the device."""
        r, _keep = _rows_struct(rows, all_columns=True)
        self._check(self.L.mkp_merge_add_rows(self.h, int(tid), ctypes.byref(r)))

    def merge_add_file(self, path, names):
        """mkp_merge_add_file: a whole bedMethyl file (plain text or bgzip) read on the device and joined run by run where its rows lie in
        HBM; names[tid] = the contig names of the table given to merge_begin (rows of another chrom are dropped and counted).  Returns the
        file's rows."""
        enc = [str(n).encode() for n in names]
        arr = (ctypes.c_char_p * max(1, len(enc)))(*enc)
        n = ctypes.c_uint64(0)
        self._check(self.L.mkp_merge_add_file(self.h, str(path).encode(), arr, len(enc), ctypes.byref(n)))
        return int(n.value)

    def read_bedmethyl_runs(self, path):
        """mkp_bedmethyl_read_device: what the module-level read_bedmethyl_runs returns, read by the device reader (inflate, line cut and
        parse on the GPU) and copied back."""
        h = ctypes.c_void_p()
        self._check(self.L.mkp_bedmethyl_read_device(self.h, str(path).encode(), ctypes.byref(h)))
        return _bedmethyl_file_runs(self.L, h)

    def merge_add_resident(self):
        """mkp_merge_add_resident: join the rows the last shard run left in HBM into their contig's table."""
        self._check(self.L.mkp_merge_add_resident(self.h))

    def merge_get(self, tid):
        """mkp_merge_get: (the merged rows of contig `tid` as rows_to_numpy gives them — motif_idx = -1 —, rows dropped since merge_begin)."""
        rows, dropped = Rows(), ctypes.c_uint64(0)
        self._check(self.L.mkp_merge_get(self.h, int(tid), ctypes.byref(rows), ctypes.byref(dropped)))
        return rows_to_numpy(rows), int(dropped.value)

    def dmr_begin(self, regions, bases=("C",), lookup=None, min_valid_coverage=0, mask=False):
        """mkp_dmr_begin: regions as stats_begin takes them; bases = the `--base` letters; lookup = {code: base letter} (None:
        MOD_CODE_TO_DNA_BASE; `--assign-code` entries are added to dmr_default_lookup()); mask = `--mask`."""
        arr, n = _region_array(regions)
        lk = dmr_default_lookup() if lookup is None else {code_repr(c): b for c, b in lookup.items()}
        codes = (ctypes.c_uint32 * max(1, len(lk)))(*lk.keys())
        cb = (ctypes.c_uint8 * max(1, len(lk)))(*["ACGT".index(b) for b in lk.values()])
        bs = "".join(bases).encode()
        self._check(self.L.mkp_dmr_begin(self.h, arr, n, bs, len(bs), codes, cb, len(lk), int(min_valid_coverage), int(bool(mask))))

    def dmr_set_reference(self, tid, seq, offset=0):
        """mkp_dmr_set_reference: seq = the reference bytes of contig tid from `offset` on; before the contig's rows."""
        b = seq if isinstance(seq, bytes) else str(seq).encode()
        self._check(self.L.mkp_dmr_set_reference(self.h, int(tid), b, int(offset), len(b)))

    def dmr_add_rows(self, sample, tid, rows):
        """mkp_dmr_add_rows: rows of ONE contig of sample 0 (a) or 1 (b), ascending pos, as a dict of arrays with all eleven columns."""
        r, _keep = _rows_struct(rows, all_columns=True)
        self._check(self.L.mkp_dmr_add_rows(self.h, int(sample), int(tid), ctypes.byref(r)))

    def dmr_add_file(self, sample, path, names):
        """mkp_dmr_add_file: a whole bedMethyl file (plain text or bgzip) of sample 0 / 1 through the device reader; names[tid]."""
        enc = [str(n).encode() for n in names]
        arr = (ctypes.c_char_p * max(1, len(enc)))(*enc)
        n = ctypes.c_uint64(0)
        self._check(self.L.mkp_dmr_add_file(self.h, int(sample), str(path).encode(), arr, len(enc), ctypes.byref(n)))
        return int(n.value)

    def dmr_add_resident(self, sample):
        """mkp_dmr_add_resident: the rows the last shard run left in HBM, as sample 0 / 1."""
        self._check(self.L.mkp_dmr_add_resident(self.h, int(sample)))

    def dmr_get(self):
        """mkp_dmr_get: {"codes": u32[k] sorted; per sample s in (0, 1): "n_mod"[s] u64[n, k], "has_code"[s] u8[n, k], "total"[s] / "n_rows"[s]
        u64[n], "bad"[s] / "contig_has_rows"[s] u8[n]; "has_reference" u8[n], "score" f64[n], "state" u8[n] (DMR_*)}."""
        o = DmrOut()
        self._check(self.L.mkp_dmr_get(self.h, ctypes.byref(o)))
        n, k, arr = int(o.n_regions), int(o.n_codes), _copy_out
        d = {"codes": arr(o.code_repr, (k,), "u4"), "has_reference": arr(o.has_reference, (n,), "u1"), "score": arr(o.score, (n,), "f8"),
             "state": arr(o.state, (n,), "u1")}
        for f, shape, dt in (("n_mod", (n, k), "u8"), ("has_code", (n, k), "u1"), ("total", (n,), "u8"), ("n_rows", (n,), "u8"), ("bad", (n,), "u1"),
                             ("contig_has_rows", (n,), "u1")):
            d[f] = [arr(getattr(o, f)[s], shape, dt) for s in range(2)]
        return d

    def dmr_sites_begin(self, contig_names, bases=("C",), lookup=None, min_valid_coverage=0, mask=False, prior=(0.55, 0.55), delta=0.05,
                        max_coverages=None, n_sample_records=10042, interval_size=100000, batch_size=6):
        """mkp_dmr_sites_begin: contig_names[tid]; bases / lookup / mask as dmr_begin; prior = Beta(alpha, beta); max_coverages = (a, b) or None
        (estimated from the first n_sample_records participating rows); interval_size / batch_size shape the reference's batches."""
        lk = dmr_default_lookup() if lookup is None else {code_repr(c): b for c, b in lookup.items()}
        enc = [str(n).encode() for n in contig_names]
        bs = "".join(bases).encode()
        cfg = DmrSitesConfig(contig_names=(ctypes.c_char_p * max(1, len(enc)))(*enc), n_contigs=len(enc), bases=bs, n_bases=len(bs),
                             codes=(ctypes.c_uint32 * max(1, len(lk)))(*lk.keys()),
                             code_bases=(ctypes.c_uint8 * max(1, len(lk)))(*["ACGT".index(b) for b in lk.values()]), n_lookup=len(lk),
                             respect_mask=int(bool(mask)), min_valid_coverage=int(min_valid_coverage), prior_alpha=float(prior[0]),
                             prior_beta=float(prior[1]), delta=float(delta), have_max_coverages=int(max_coverages is not None),
                             n_sample_records=int(n_sample_records), interval_size=int(interval_size), batch_size=int(batch_size))
        if max_coverages is not None:
            cfg.max_coverages[0], cfg.max_coverages[1] = int(max_coverages[0]), int(max_coverages[1])
        self._check(self.L.mkp_dmr_sites_begin(self.h, ctypes.byref(cfg)))

    def dmr_sites_set_reference(self, tid, seq):
        """mkp_dmr_sites_set_reference: seq = the whole sequence of contig tid."""
        b = seq if isinstance(seq, bytes) else str(seq).encode()
        self._check(self.L.mkp_dmr_sites_set_reference(self.h, int(tid), b, len(b)))

    def dmr_sites_add_rows(self, sample, tid, rows):
        """mkp_dmr_sites_add_rows: rows of ONE contig of sample 0 (a) or 1 (b), ascending pos, as a dict of arrays with all eleven columns."""
        r, _keep = _rows_struct(rows, all_columns=True)
        self._check(self.L.mkp_dmr_sites_add_rows(self.h, int(sample), int(tid), ctypes.byref(r)))

    def dmr_sites_add_file(self, sample, path):
        """mkp_dmr_sites_add_file: a whole bedMethyl file (plain text or bgzip) of sample 0 / 1 through the device reader; returns its rows."""
        n = ctypes.c_uint64(0)
        self._check(self.L.mkp_dmr_sites_add_file(self.h, int(sample), str(path).encode(), ctypes.byref(n)))
        return int(n.value)

    def dmr_sites_get(self):
        """mkp_dmr_sites_get: {"codes": u32[k] sorted; per written site "tid" i32[n], "pos" u32[n], "strand" (str of '+' / '-'), "score" /
        "map_pvalue" / "effect_size" f64[n]; per sample s in (0, 1): "total"[s] u32[n], "n_mod"[s] u32[n, k], "has_code"[s] u32[n] (column
        masks); "max_coverages" (a, b), "n_sampled" (a, b), "n_batches", "n_batches_dropped", "n_model_failures"}."""
        o = DmrSitesOut()
        self._check(self.L.mkp_dmr_sites_get(self.h, ctypes.byref(o)))
        n, k, arr = int(o.n_sites), int(o.n_codes), _copy_out
        d = {"codes": arr(o.code_repr, (k,), "u4"), "tid": arr(o.tid, (n,), "i4"), "pos": arr(o.pos, (n,), "u4"),
             "strand": arr(o.strand, (n,), "u1").tobytes().decode(), "score": arr(o.score, (n,), "f8"), "map_pvalue": arr(o.map_pvalue, (n,), "f8"),
             "effect_size": arr(o.effect_size, (n,), "f8"), "max_coverages": (int(o.max_coverages[0]), int(o.max_coverages[1])),
             "n_sampled": (int(o.n_sampled[0]), int(o.n_sampled[1])), "n_batches": int(o.n_batches), "n_batches_dropped": int(o.n_batches_dropped),
             "n_model_failures": int(o.n_model_failures)}
        for f, shape in (("total", (n,)), ("n_mod", (n, k)), ("has_code", (n,))):
            d[f] = [arr(getattr(o, f)[s], shape, "u4") for s in range(2)]
        return d

    def dmr_reps_begin(self, contig_names, n_a, n_b, bases=("C",), lookup=None, min_valid_coverage=0, mask=False, prior=(0.55, 0.55), delta=0.05,
                       max_coverages=None, n_sample_records=10042, interval_size=100000, batch_size=6, cap_coverages=False):
        """mkp_dmr_reps_begin: n_a / n_b = the tables of a side (1 .. 16); the max coverages (given or estimated) are multiplied by the side's
        number of tables unless cap_coverages, then capped at 300; everything else as dmr_sites_begin."""
        lk = dmr_default_lookup() if lookup is None else {code_repr(c): b for c, b in lookup.items()}
        enc = [str(n).encode() for n in contig_names]
        bs = "".join(bases).encode()
        cfg = DmrSitesConfig(contig_names=(ctypes.c_char_p * max(1, len(enc)))(*enc), n_contigs=len(enc), bases=bs, n_bases=len(bs),
                             codes=(ctypes.c_uint32 * max(1, len(lk)))(*lk.keys()),
                             code_bases=(ctypes.c_uint8 * max(1, len(lk)))(*["ACGT".index(b) for b in lk.values()]), n_lookup=len(lk),
                             respect_mask=int(bool(mask)), min_valid_coverage=int(min_valid_coverage), prior_alpha=float(prior[0]),
                             prior_beta=float(prior[1]), delta=float(delta), have_max_coverages=int(max_coverages is not None),
                             n_sample_records=int(n_sample_records), interval_size=int(interval_size), batch_size=int(batch_size))
        if max_coverages is not None:
            cfg.max_coverages[0], cfg.max_coverages[1] = int(max_coverages[0]), int(max_coverages[1])
        self._check(self.L.mkp_dmr_reps_begin(self.h, ctypes.byref(cfg), int(n_a), int(n_b), int(bool(cap_coverages))))

    def dmr_reps_set_reference(self, tid, seq):
        """mkp_dmr_reps_set_reference: seq = the whole sequence of contig tid."""
        b = seq if isinstance(seq, bytes) else str(seq).encode()
        self._check(self.L.mkp_dmr_reps_set_reference(self.h, int(tid), b, len(b)))

    def dmr_reps_add_rows(self, side, replicate, tid, rows):
        """mkp_dmr_reps_add_rows: rows of ONE contig of table `replicate` of side 0 (a) or 1 (b), ascending pos, a dict of arrays with all eleven
        columns."""
        r, _keep = _rows_struct(rows, all_columns=True)
        self._check(self.L.mkp_dmr_reps_add_rows(self.h, int(side), int(replicate), int(tid), ctypes.byref(r)))

    def dmr_reps_add_file(self, side, replicate, path):
        """mkp_dmr_reps_add_file: a whole bedMethyl file (plain text or bgzip) through the device reader; returns its rows."""
        n = ctypes.c_uint64(0)
        self._check(self.L.mkp_dmr_reps_add_file(self.h, int(side), int(replicate), str(path).encode(), ctypes.byref(n)))
        return int(n.value)

    def dmr_reps_get(self):
        """mkp_dmr_reps_get: the dict of dmr_sites_get over the collapsed counts, and "n_a", "n_b", "balanced_map_pvalue" / "balanced_effect_size"
        f64[n], "pct_samples" (u32[n], u32[n]), "n_rep" u32[n] and, with matched sides, "rep_pvalue" / "rep_effect" f64[n, n_a] (row i holds
        n_rep[i] values); otherwise those two are None."""
        o = DmrRepsOut()
        self._check(self.L.mkp_dmr_reps_get(self.h, ctypes.byref(o)))
        t = o.sites
        n, k, arr = int(t.n_sites), int(t.n_codes), _copy_out
        d = {"codes": arr(t.code_repr, (k,), "u4"), "tid": arr(t.tid, (n,), "i4"), "pos": arr(t.pos, (n,), "u4"),
             "strand": arr(t.strand, (n,), "u1").tobytes().decode(), "score": arr(t.score, (n,), "f8"), "map_pvalue": arr(t.map_pvalue, (n,), "f8"),
             "effect_size": arr(t.effect_size, (n,), "f8"), "max_coverages": (int(t.max_coverages[0]), int(t.max_coverages[1])),
             "n_sampled": (int(t.n_sampled[0]), int(t.n_sampled[1])), "n_batches": int(t.n_batches), "n_batches_dropped": int(t.n_batches_dropped),
             "n_model_failures": int(t.n_model_failures), "n_a": int(o.n_a), "n_b": int(o.n_b),
             "balanced_map_pvalue": arr(o.balanced_map_pvalue, (n,), "f8"), "balanced_effect_size": arr(o.balanced_effect_size, (n,), "f8"),
             "pct_samples": tuple(arr(o.pct_samples[s], (n,), "u4") for s in range(2)), "n_rep": arr(o.n_rep, (n,), "u4")}
        for f, shape in (("total", (n,)), ("n_mod", (n, k)), ("has_code", (n,))):
            d[f] = [arr(getattr(t, f)[s], shape, "u4") for s in range(2)]
        matched = o.n_a == o.n_b and o.n_a > 1
        d["rep_pvalue"] = arr(o.rep_pvalue, (n, int(o.n_a)), "f8") if matched else None
        d["rep_effect"] = arr(o.rep_effect, (n, int(o.n_a)), "f8") if matched else None
        return d

    def rerun(self, iters, fetch=False):
        rows = Rows()
        self._check(self.L.mkp_shard_rerun(self.h, int(iters), ctypes.byref(rows) if fetch else None))
        return rows

    def read_flags(self):
        """the packer's flags of the reads of the open / resident shard, file order (READ_WIDE_CIGAR: mkp_shard_read_flags)"""
        n = ctypes.c_uint32(0)
        self._check(self.L.mkp_shard_read_flags(self.h, None, 0, ctypes.byref(n)))
        buf = (ctypes.c_uint32 * max(n.value, 1))()
        self._check(self.L.mkp_shard_read_flags(self.h, buf, n.value, ctypes.byref(n)))
        return list(buf[:n.value])

    def stats(self):
        s = Stats()
        self._check(self.L.mkp_get_stats(self.h, ctypes.byref(s)))
        return s


ROW_FIELDS = ("pos", "strand", "code_repr", "motif_idx", "n_valid", "n_mod", "n_canonical", "n_other", "n_delete", "n_fail", "n_diff", "n_nocall")


def read_bedmethyl(path):
    """The count columns of a bedMethyl file (writers.rs:87-156) as the row arrays mkp_rows carries: pos, strand, code_repr (a letter's
    code point, or the ChEBI number | 1 << 31), n_valid, n_mod, n_canonical, n_other, n_delete, n_fail, n_diff, n_nocall — so that rows
    fetched from the device can be compared with a file that was itself compared with the oracle's."""
    import numpy as np
    import pandas as pd
    cols = {1: "pos", 3: "code", 5: "strand", 9: "n_valid", 11: "n_mod", 12: "n_canonical", 13: "n_other", 14: "n_delete", 15: "n_fail", 16: "n_diff", 17: "n_nocall"}
    if os.path.getsize(path) == 0:
        return {f: np.zeros(0, dtype=np.uint32) for f in ROW_FIELDS if f != "motif_idx"}
    df = pd.read_csv(path, sep=r"\s+", header=None, usecols=sorted(cols), dtype={3: str, 5: str}, engine="c")
    out = {name: df[k].to_numpy().astype(np.uint32) for k, name in cols.items() if name not in ("code", "strand")}
    out["strand"] = df[5].map(ord).to_numpy().astype(np.uint8)
    out["code_repr"] = df[3].map(lambda c: (int(c) | (1 << 31)) if c.isdigit() else ord(c)).to_numpy().astype(np.uint32)
    return out


def rows_digest(r, fields=("pos", "strand", "code_repr", "n_valid", "n_mod", "n_canonical", "n_other", "n_delete", "n_fail", "n_diff", "n_nocall")):
    """sha256 over the row arrays (numpy dicts from rows_to_numpy / read_bedmethyl), field by field, widths normalised."""
    import hashlib
    import numpy as np
    h = hashlib.sha256()
    for f in fields:
        h.update(np.ascontiguousarray(np.asarray(r[f]).astype(np.uint32)).tobytes())
    return h.hexdigest()


def rows_to_numpy(rows):
    """Copy an mkp_rows view (owned by the ctx until its next run) into a dict of numpy arrays."""
    import numpy as np
    n = int(rows.n_rows)
    out = {}
    for f in ROW_FIELDS:
        p = getattr(rows, f)
        out[f] = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint32)
    return out


def read_bedmethyl_for_stats(path):
    """What `stats` reads of a bedMethyl file: plain text (not bgzip-compressed), no header line, columns separated by tabs and / or blanks
    (both the default and the --mixed-delim form): column 1 chrom, 2 start, 4 name — the mod code is the name up to its first comma, so the
    `m,CG,0` names of multi-motif runs are taken too —, 6 strand, 10 N_valid_cov, 12 N_mod (BedMethylLine, src/dmr/bedmethyl.rs:40-86).
    Returns [(chrom, rows dict), ...]: one entry per run of lines on one contig, file order."""
    import numpy as np
    import pandas as pd
    if os.path.getsize(path) == 0:
        return []
    df = pd.read_csv(path, sep=r"\s+", header=None, usecols=[0, 1, 3, 5, 9, 11], dtype={0: str, 3: str, 5: str}, engine="c")
    chrom = df[0].to_numpy()
    cut = [0] + [i for i in range(1, len(chrom)) if chrom[i] != chrom[i - 1]] + [len(chrom)]
    code = df[3].map(lambda c: code_repr(c.split(",", 1)[0])).to_numpy().astype(np.uint32)
    strand = df[5].map(ord).to_numpy().astype(np.uint8)
    out = []
    for a, b in zip(cut[:-1], cut[1:]):
        out.append((chrom[a], {"pos": df[1].to_numpy()[a:b].astype(np.uint32), "strand": strand[a:b], "code_repr": code[a:b],
                               "n_valid": df[9].to_numpy()[a:b].astype(np.uint32), "n_mod": df[11].to_numpy()[a:b].astype(np.uint32)}))
    return out


def stats(bedmethyl_path, regions_bed, out_table, codes=None, min_coverage=1, header=True, device=0):
    """`modkit stats <bedmethyl> --regions <bed> -o <table>` (EntryStats::run, src/stats/subcommand.rs:65-206) on the device: the file's rows
    are uploaded contig by contig and reduced by the kernels a fused `pileup --region-stats` run uses (Context.stats_add_rows).  Reads what
    read_bedmethyl_for_stats reads: a PLAIN-TEXT bedMethyl without header (no bgzip / tabix needed); a region whose contig has no line in
    the file is dropped, as the reference drops contigs its tabix index does not list.  codes = `--mod-codes`, header=False = `--no-header`."""
    pieces = read_bedmethyl_for_stats(bedmethyl_path)
    names = []
    for chrom, _ in pieces:
        if chrom not in names:
            names.append(chrom)
    rs = RegionSet(regions_bed, names)
    ctx = Context(device=device)
    try:
        ctx.stats_begin(rs, codes=codes, min_coverage=min_coverage)
        for chrom, rows in pieces:
            ctx.stats_add_rows(names.index(chrom), rows)
        rs.write_table(ctx.stats_get(), out_table, header=header)
    finally:
        ctx.close()
        rs.close()


def localize(bedmethyl_path, regions_bed, genome_sizes_path, out_table, window=2000, stranded=None, stranded_features=None, device=0):
    """`modkit localize <bedmethyl> --regions <bed> --genome-sizes <tsv> -o <table>` (EntryLocalize::run, src/localise/subcommand.rs:211-305) on
    the device: the file's rows are uploaded contig by contig and go through the kernels a fused `pileup --localize` run uses
    (Context.localize_add_rows).  Reads what read_bedmethyl_for_stats reads: a PLAIN-TEXT bedMethyl without header; a region whose contig is
    not in the sizes file or has no line in the bedMethyl is dropped.  window = `--window`, stranded = `--stranded` ("same" / "opposite"),
    stranded_features = `--stranded-features` ("+", "-", ".").  There is no min_coverage: the reference only logs it."""
    pieces = read_bedmethyl_for_stats(bedmethyl_path)
    sizes = genome_sizes(genome_sizes_path)
    names = [n for n, _ in sizes]
    n_sized = len(names)
    for chrom, _ in pieces:          # (contigs of the file that the sizes do not list: their rows bring nothing, no region can be on them)
        if chrom not in names:
            names.append(chrom)
    rs = RegionSet(regions_bed, names[:n_sized], localize=True)
    ctx = Context(device=device)
    try:
        ctx.localize_begin(rs, [l for _, l in sizes], window=window, stranded=stranded, stranded_features=stranded_features)
        for chrom, rows in pieces:
            ctx.localize_add_rows(names.index(chrom), rows)
        write_localize_table(ctx.localize_get(), out_table)
    finally:
        ctx.close()
        rs.close()
