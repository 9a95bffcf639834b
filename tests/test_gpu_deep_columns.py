"""GPU: columns deeper than 65 535 records.  The packed tallies hold a strand's count in 16 bits; a shard whose deepest column may exceed that
runs the wide-tally accumulate kernels (depth_guard, mkp_plan.hpp) and must equal the oracle byte for byte.  pileup-hemi has no wide kernel
and refuses such a shard loudly."""
import os
import subprocess

import pytest

import modkit_amd
from deep_column_cases import amplicon_key, amplicon_records, background_records, reference, stack_records, write_bam, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "modkit_amd", "csrc", "mkpileup")
DEEP = ["--max-depth", "100000", "--filter-threshold", "0.7"]
AMP_AT, AMP_FWD = 1000, 70000


@pytest.fixture(scope="module")
def amplicon(tmp_path_factory):
    """70 000 forward + 3 000 reverse reads of 300 bp over one locus with CpGs, C+m? / C+hm?, deletions and ref-skips; indexed."""
    d = tmp_path_factory.mktemp("amplicon")
    ref = reference(4000)
    recs = amplicon_records(ref, AMP_AT, AMP_FWD, 3000, keys=True)
    bam = write_bam(str(d / "amp"), ("ctg", 4000), recs, index=True)
    parts = {str(key): write_bam(str(d / ("amp_hp%d" % key)), ("ctg", 4000), [r for k, r in enumerate(recs) if amplicon_key(k, AMP_FWD) == key])
             for key in (1, 2)}
    return bam, write_fasta(str(d / "amp.fa"), "ctg", ref), parts


def oracle(oracle_bin, bam, out, flags):
    p = subprocess.run([oracle_bin, "pileup", bam, out] + flags, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-300:]
    return open(out).read()


def both(oracle_bin, tmp_path, bam, flags):
    dev, ora = str(tmp_path / "dev.bed"), str(tmp_path / "ora.bed")
    modkit_amd.pileup([bam, dev] + flags)
    want = oracle(oracle_bin, bam, ora, flags)
    got = open(dev).read()
    assert want and got == want
    return got


def deepest(bed):
    return max(int(ln.split("\t")[9]) for ln in bed.splitlines())


@pytest.mark.parametrize("mode", ["cpg", "dense", "cpg_combine", "cpg_interval"])
def test_amplicon_pile_vs_oracle(oracle_bin, tmp_path, amplicon, mode):
    bam, fa, _ = amplicon
    flags = {"cpg": ["--cpg", "--ref", fa], "dense": [], "cpg_combine": ["--cpg", "--ref", fa, "--combine-strands"],
             "cpg_interval": ["--cpg", "--ref", fa, "-i", "1100"]}[mode]   # the pile [1000, 1340) straddles the interval start 1100
    got = both(oracle_bin, tmp_path, bam, flags + DEEP)
    assert deepest(got) > 65535


def test_amplicon_partition_tags_vs_oracle_on_split_bams(oracle_bin, tmp_path, amplicon):
    # one pass per HP key (the _keyed_wide kernels); every key's file equals the oracle's unpartitioned pileup of that key's reads alone.
    # Key 1 holds 67 813 forward reads and the 3 000 reverse ones: a '+' tally over 16 bits would carry into the '-' rows
    bam, fa, parts = amplicon
    flags = ["--cpg", "--ref", fa] + DEEP
    out_dir = str(tmp_path / "parts")
    modkit_amd.pileup([bam, out_dir, "--partition-tag", "HP", "--prefix", "hap"] + flags)
    assert sorted(os.listdir(out_dir)) == ["hap_1.bed", "hap_2.bed"]
    for key, sub in parts.items():
        want = oracle(oracle_bin, sub, str(tmp_path / ("ora_%s.bed" % key)), flags)
        got = open(os.path.join(out_dir, "hap_%s.bed" % key)).read()
        assert want and got == want, key
    assert deepest(open(os.path.join(out_dir, "hap_1.bed")).read()) > 65535


@pytest.mark.parametrize("n", [65535, 65536])
def test_boundary_column_vs_oracle_and_stats(oracle_bin, tmp_path, n):
    # exactly 65 535 forward reads over a column still fit the 16-bit halves; one more takes the wide kernels, and --stats says so
    ref = reference(1000)
    bam = write_bam(str(tmp_path / "stack"), ("ctg", 1000), stack_records(ref, 200, n))
    fa = write_fasta(str(tmp_path / "stack.fa"), "ctg", ref)
    for flags in ([], ["--cpg", "--ref", fa]):
        dev, ora = str(tmp_path / "dev.bed"), str(tmp_path / "ora.bed")
        p = subprocess.run([CLI, "pileup", bam, dev, "--stats"] + flags + DEEP, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-300:]
        want = oracle(oracle_bin, bam, ora, flags + DEEP)
        assert want and open(dev).read() == want
        assert deepest(want) == n
        assert ("wide tallies: 1 of 1 shards" in p.stderr) == (n > 65535), p.stderr[-600:]


def test_deep_amplicon_inside_ordinary_coverage(oracle_bin, tmp_path):
    # one shard: ~30x background over a 20 kb contig and a 68 000-read amplicon (66 000 forward) in its middle
    ref = reference(20000, seed=23)
    recs = background_records(ref, 20000, 30, first=1000000) + amplicon_records(ref, 9000, 66000, 2000)
    bam = write_bam(str(tmp_path / "mixed"), ("ctg", 20000), recs)
    fa = write_fasta(str(tmp_path / "mixed.fa"), "ctg", ref)
    for flags in ([], ["--cpg", "--ref", fa]):
        got = both(oracle_bin, tmp_path, bam, flags + DEEP)
        assert deepest(got) > 65535 and len(got.splitlines()) > 1000


@pytest.mark.parametrize("mode", ["cpg", "dense"])
def test_deep_shard_relaunch_returns_first_pass(oracle_bin, tmp_path, amplicon, mode):
    # what a timed re-launch launches is what the shard pass launched: the wide kernels, with the oracle's rows
    bam, fa, _ = amplicon
    flags = (["--cpg", "--ref", fa] if mode == "cpg" else []) + DEEP
    ora, dev = str(tmp_path / "ora.bed"), str(tmp_path / "dev.bed")
    assert oracle(oracle_bin, bam, ora, flags)
    want = modkit_amd.rows_digest(modkit_amd.read_bedmethyl(ora))
    ctx = modkit_amd.Context(device=0)
    try:
        rep = ctx.pileup_run([bam, dev] + flags + ["--shard-bytes", str(1 << 40)])
        assert rep.n_shards == 1 and open(dev).read() == open(ora).read()
        assert modkit_amd.rows_digest(modkit_amd.rows_to_numpy(ctx.rerun(0, fetch=True))) == want
        assert modkit_amd.rows_digest(modkit_amd.rows_to_numpy(ctx.rerun(2, fetch=True))) == want
    finally:
        ctx.close()


def test_hemi_deeper_than_16_bits_is_refused(tmp_path, amplicon):
    bam, fa, _ = amplicon
    out = str(tmp_path / "hemi.bed")
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.pileup_hemi([bam, "-o", out, "--cpg", "-r", fa, "--max-depth", "100000", "--no-filtering"])
    assert e.value.status == -3 and "more than 65535 reads over one position" in str(e.value)
    assert not os.path.exists(out) or os.path.getsize(out) == 0
