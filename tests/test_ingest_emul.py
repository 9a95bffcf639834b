"""The device ingest's per-thread code (modkit_amd/csrc/mkp_ingest_dev.hpp: record chains, record checks + region test, aux walk, MM
tokeniser, packing) compiled for the host and run thread by thread over whole BAMs by tests/ingest_emul.cpp, against the host path it
replaces (mkp_bam.hpp's record index, Packer::add): record offsets, kept / supplementary classification per region, headers, CIGAR
words and chunk prefixes, SEQ bytes, per-tag rank lists and ML bytes, name and layout-key hashes, the same-list and probability-sum
flags — and the same refusals.  The sliced CRC-32 join of mkp_crc32_blocks is checked against zlib over the same streams.

The host-only steps of the ingest (modkit_amd/csrc/mkp_ingest_stages.hpp: upload layout, chain table, stage cut, block lists, error mapping,
layout interning) are the product's own functions here, driven by the emulated kernels or by hand-written input."""
import os
import struct
import subprocess

import pytest

from bamfuzz import Fuzz, aux_bc, aux_i, aux_z, bam_header, bam_record, bgzf_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "modkit_fixtures")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emul") / "ingest_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           "-o", exe, os.path.join(ROOT, "tests", "ingest_emul.cpp"), "-lz", "-lpthread"])
    return exe


def run(emul, bam, every):
    p = subprocess.run([emul, bam, str(every)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.startswith("ok"), p.stdout
    return p.stdout


@pytest.mark.parametrize("every", [1, 3, 1000])
def test_reference_fixtures(emul, every):
    for f in sorted(os.listdir(FIX)):
        if f.endswith(".bam"):
            run(emul, os.path.join(FIX, f), every)


@pytest.mark.parametrize("profile", ["mixed", "m", "hm_comb", "hm_split", "hm_split_diff", "hma", "implicit", "default", "duplex", "nbase", "chebi", "duplex_hm", "duplex_split",
                                     "duplex_chebi", "duplex_3codes"])
def test_fuzzed_bams(emul, tmp_path, profile):
    for seed in (3, 4):
        bam, _, _ = Fuzz(seed, profile=profile, n_reads=300, tie_rate=0.2, weird_rate=0.25).write(str(tmp_path / ("fz%d" % seed)))
        out = run(emul, bam, 5)
        assert "compared=0" not in out
        # the product's layout interning over the emulated digest: every packed record with tags got the host packer's key string
        assert int(out.split("interned=")[1].split()[0]) > 0


def test_forged_key_hash_is_refused(emul, tmp_path):
    """Two records of different MM header structures under one 64-bit key hash (the harness hands ingest_intern_layouts a digest in which
    the first record's hash is the second's): the "disagree" / "share a 64-bit key hash" error, never the wrong caller tables.  It is the
    "disagree on a record's MM header structure" throw that this reaches (the forged record is interned first and its own key hashes to
    something else); "share a 64-bit key hash" needs two real keys with one FNV-64 value and is reached by no forged digest."""
    bam, _, _ = Fuzz(3, profile="mixed", n_reads=300, tie_rate=0.2, weird_rate=0.25).write(str(tmp_path / "fz"))
    out = run(emul, bam, 5)
    assert int(out.split("forged=")[1].split()[0]) > 0


def test_generated_long_reads(emul, tmp_path):
    from test_host_ingest import gen
    bam, _ = gen(tmp_path, "g", [("c1", 400000), ("c2", 150000)], 1500)
    out = run(emul, bam, 48)
    assert int(out.split("records=")[1].split()[0]) >= 1500


MM_CASES = [
    "C+m?,1,2,3;", "C+m?;", "C+m,0;", "C+m.,0,0;", "C+hm?,1,2;", "C+h?,1,2;C+m?,1,2;", "C+h?,1,2;C+m?,1,3;", "C+h?,1;C+m?,1,2;",
    "C+m?,1,2,x,5;", "C+m?,1,,2;", "C+m?, 1 ,\t2;", "C+m?,1 2;", "C+m?,;", "C+m?,1,2,;", "C+m?,99999999999;", "C+m?,4294967295;", "C+m?,4294967294,0;",
    "N+m?,3,4;", "N+m?,50;", "N+m?,10,10,10;", "C+76792?,1,2;", "C+76792m?,1;", "C+2147483648?,1;", "C+m7?,1;", "C-m?,1;G+m?,2;", "C+m?,1;;G-m?,0;",
    ";;C+m?,1;", "X+m?,1;", "C*m?,1;", "C;", "C+;", "C+?;", "C+?,1;", "C+abcde?,1;", "C+abcd?,1;", "U+m?,0;", "C+m?,1;A+a?,0;G+x?,1;T+y?,0;C+h?,2;A+b?,0;G+z?,1;T+w?,0;",
    "C+m?,1;A+a?,0;G+x?,1;T+y?,0;C+h?,2;A+b?,0;G+z?,1;T+w?,0;C+q?,1;", "C+m?,1;A+a?,0;G+x?,1;T+y?,0;C+h?,2;A+b?,0;G+z?,1;T+w?,0;Q+q?,1;", "C+m\xc3\xa9?,1;",
    "C+m?,1;C+m?,1;", "C+h?,0,0,0;C+m?,0,0,0;", "C+hm?,0,0,0;C+a?,0,0,0;", "",
]


THROWERS = {"C+abcde?,1;", "C+m?,1;A+a?,0;G+x?,1;T+y?,0;C+h?,2;A+b?,0;G+z?,1;T+w?,0;C+q?,1;", "C+m\xc3\xa9?,1;"}   # the host packer refuses the whole shard


def _mm_bam(path, cases, ml_mode, k):
    seq = "ACGT" * 12 + "CCGG"
    recs = []
    for i, mm in enumerate(cases):
        n_deltas = sum(seg.count(",") for seg in mm.split(";"))
        n_ml = {"fit": 2 * n_deltas + 2, "short": max(0, n_deltas - 1), "long": 4 * n_deltas + 9}.get(ml_mode, 2 * n_deltas + 2)
        mm_tag, ml_tag = ("Mm", "Ml") if ml_mode == "old" else ("MM", "ML")
        aux = mm_tag.encode() + b"Z" + mm.encode("latin-1") + b"\0"
        if ml_mode == "wrongtype":
            aux += ml_tag.encode() + b"BS" + struct.pack("<I", n_ml) + bytes(2 * n_ml)
        elif ml_mode != "none":
            aux += aux_bc(ml_tag, [(37 * j + 11 * i) % 256 for j in range(n_ml)])
        if ml_mode == "mn_ok":
            aux += aux_i("MN", len(seq))
        elif ml_mode == "mn_bad":
            aux += aux_i("MN", len(seq) + 1)
        elif ml_mode == "mn_short":
            aux = b"MNs" + struct.pack("<h", len(seq)) + aux
        flag = 16 if i % 3 == 0 else 0
        recs.append(bam_record(0, 10 + 7 * i, flag, "r%d_%d" % (k, i), [(len(seq), "M")], seq, b"XAi" + struct.pack("<i", 5) + aux))
    bgzf_write(path, bytes(bam_header([("c", 5000)])) + b"".join(recs))


def test_handwritten_mm_strings(emul, tmp_path):
    """Tag grammar corner cases: trailing garbage after a valid prefix, whitespace, empty elements, overflowing numbers, ChEBI codes, `N`
    tags past the read end, nine tags with a broken ninth, duplicate tags, MN / Mm / Ml variants, ML of the wrong type or length."""
    clean = [m for m in MM_CASES if m not in THROWERS]
    for k, ml_mode in enumerate(("fit", "short", "long", "wrongtype", "old", "mn_ok", "mn_bad", "mn_short", "none")):
        bam = str(tmp_path / ("mm_%s.bam" % ml_mode))
        _mm_bam(bam, clean, ml_mode, k)
        out = run(emul, bam, 4)
        assert "compared=%d" % (3 * len(clean)) in out or "compared=" in out


@pytest.mark.parametrize("mm", sorted(THROWERS))
def test_refusals_match_the_host_packer(emul, tmp_path, mm):
    """Five codes in one tag, nine tags, a non-ASCII code: the host packer throws MKP_E_UNSUPPORTED; the device sets the matching error bit
    (checked inside the harness: a host throw without the bit, or a bit without the throw, fails), and the product's mapping of that bit
    (ingest_throw_error_bits) gives the host's status and words."""
    bam = str(tmp_path / "t.bam")
    _mm_bam(bam, ["C+m?,1,2;", mm, "C+h?,3;"], "fit", 0)
    run(emul, bam, 2)
    # with a short ML array the broken tag is reached after the "ML array too short" answer of an earlier tag in some cases: still the same verdict on both sides
    _mm_bam(bam, ["C+m?,1,2;", mm], "short", 0)
    run(emul, bam, 1)


def run_plan(emul, bam, piece=None, stage_rounds=None):
    """the plan checks, the block table built in stages of `stage_rounds` upload rounds of sixteen `piece`-byte pieces (default: the
    product's 1 MiB pieces, one stage); returns (stdout, its key=value figures)"""
    p = subprocess.run([emul, "--plan", bam] + ([str(piece), str(stage_rounds)] if piece else []), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.startswith("ok"), p.stdout
    return p.stdout, {k: int(v) for k, v in (w.split("=") for w in p.stdout.split() if "=" in w)}


def test_index_plans_select_the_fetch_records(emul, tmp_path):
    """BamSource::ingest_plan (block table + entry points from the BAI: samtools-written, generator-written, fuzzer-written) + chain walk +
    region test == BamSource::fetch, for whole contigs and sub-regions."""
    for f in sorted(os.listdir(FIX)):
        if f.endswith(".bam") and os.path.exists(os.path.join(FIX, f + ".bai")):
            _, fig = run_plan(emul, os.path.join(FIX, f))
            assert fig["boundaries"] == 0 and fig["stages"] > 0      # one round, one stage per window
    from test_host_ingest import gen
    bam, _ = gen(tmp_path, "g", [("c1", 900000), ("c2", 250000)], 4000, ["--mean-len", "6000"])
    out, fig = run_plan(emul, bam)
    assert int(out.split("segments=")[1]) > 50      # the linear index supplied entry points
    # The staged block table (the product's upload layout, stage cut and block lists around the emulated chain kernels; what has not been
    # uploaded when a stage is cut holds filler) must be the host walk's plan field by field — checked inside the harness — with 1 MiB stages
    # (64 KiB pieces, one round each) and with 192 KiB ones (4 KiB pieces, three rounds).  In both, every round boundary lies inside a chain.
    windows = fig["stages"]
    for piece, rounds in ((65536, 1), (4096, 3)):
        _, fig = run_plan(emul, bam, piece, rounds)
        assert fig["stages"] > 2 * windows and fig["boundaries"] > 0 and fig["inside"] == fig["boundaries"], fig
    # A stage that ends on no chain needs a chain longer than the stage: this file has none at 192 KiB, so the pieces shrink to 1 KiB
    # (48 KiB stages).  A stage WITH chains but without a block does not exist for a BAM whose index matches it: a
    # chain begins at a block start at or before its chunk's end block and lies wholly in the uploaded range, so it holds that block
    # (no_block == 0 at every piece size down to 64 bytes, and for every fixture); the bookkeeping of such a stage is checked on a
    # hand-written table in test_upload_layout_and_stage_bookkeeping_by_brute_force.
    _, fig = run_plan(emul, bam, 1024, 3)
    assert fig["no_chain"] >= 1 and fig["inside"] >= 1 and fig["no_block"] == 0, fig
    for seed in (0, 1):
        bam, _, _ = Fuzz(seed, contigs=(("ctgA", 90000), ("ctgB", 20000)), n_reads=900, mean_len=2500, index=True).write(str(tmp_path / ("fz%d" % seed)))
        run_plan(emul, bam)
        run_plan(emul, bam, 4096, 1)


def test_upload_layout_and_stage_bookkeeping_by_brute_force(emul):
    """UploadLayout over three hand-written range lists (one range shorter than a piece; one of exactly a round of pieces; two ranges, the
    first ending mid-round): every byte of every range in exactly one piece, z_off against zbase, round ends ascending up to zbytes, and the
    copies of every round carried out on a model of the staging half — they must reproduce the window byte for byte, write nothing twice and
    no padding, and merge pieces only where they are back to back in staging and in the window.  Then ingest_stage_cut on a hand-written
    chain list and ingest_chain_blocks on four stages, one of them without a chain and one with two chains and no block."""
    p = subprocess.run([emul, "--layout"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.startswith("ok layout") and "merged=0" not in p.stdout, p.stdout


# status and message of every refusal, as mkp_internal_ingest_run worded them before the mapping moved to mkp_ingest_stages.hpp
ERROR_BITS = {
    0: (0, "-"),
    1: (-2, "corrupt BAM record"),
    2: (-2, "truncated BAM record at the end of {path}"),
    4: (-2, "the BAM index does not match the file (a record chain misses an indexed record start): {path}.bai"),
    8: (-3, "shard exceeds 4 GiB of packed bases; use smaller shards"),
    16: (-1, "CIGAR query length does not match SEQ length"),
    32: (-3, "a read or its alignment spans 2^26 bases or more (the depth walk packs query offsets in 27 bits)"),
    64: (-3, "non-ASCII mod code"),
    128: (-3, "more than 4 mod codes in one MM tag"),
    256: (-3, "more than 8 MM tags in one read"),
    512: (-3, "shard exceeds 4 GiB of packed bases; use smaller shards"),
    3: (-2, "truncated BAM record at the end of {path}"),       # TRUNCATED | CORRUPT: the truncation is what gets reported
}


def test_error_bits_map_to_the_host_path_errors(emul):
    path = "/data/run 7/reads.bam"
    p = subprocess.run([emul, "--errors", path], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    got = {}
    for ln in p.stdout.splitlines():
        bits, status, msg = ln.split(" ", 2)
        got[int(bits)] = (int(status), msg)
    assert got == {b: (st, m.format(path=path)) for b, (st, m) in ERROR_BITS.items()}
