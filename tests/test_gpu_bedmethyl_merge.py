"""`bedmethyl merge` on the device (mkp_merge.hip behind mkp_merge_begin / _add_rows / _add_resident / _get, `mkpileup bedmethyl merge` and
`modkit pileup --merge-bedmethyl`) against the independent model of tests/bedmethyl_merge_model.py.
1. directed add_rows cases in units of T = mkp_merge_tile_rows(): empty sides, one side wholly before / behind the other, interleaved,
   identical, runs of equal keys on and across a tile edge, every strand with ChEBI and letter codes at one position, twenty codes;
2. counts at the 32-bit limit, rows beyond the contig, a three-way fold in every order, a seeded fuzz over two contigs, misuse;
3. fused runs: the output of `pileup --merge-bedmethyl prior` must equal, byte for byte, the model's merge of the same run's plain output
   with the prior files; the stand-alone subcommand on three files; 4. the refusals."""
import gzip
import itertools
import os
import struct

import numpy as np
import pytest

import modkit_amd
import bedmethyl_merge_model as model
from pileup_cases import FIX, REF, hemi_reference_fasta

pytestmark = pytest.mark.gpu

BC = os.path.join(FIX, "bc_anchored_10_reads.sorted.bam")
HG = os.path.join(FIX, "HG002_small.ch20._other.sorted.bam")
U32 = (1 << 32) - 1
T = modkit_amd.merge_tile_rows()
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7]
INVALID, IO, UNSUPPORTED = -1, -2, -3
FIELDS = ("pos", "strand", "code_repr") + model.COUNTS


@pytest.fixture(scope="module")
def ctx():
    c = modkit_amd.Context()
    yield c
    c.close()


# ---- 1. directed rows
def make_rows(n, seed, lo=0, gap=3, codes=("m", "h", "21839")):
    """n rows of one contig: ascending positions with repeats, in drawn (unsorted) order inside a position, every strand; keys repeat
    where the draw repeats them"""
    rng = np.random.default_rng(seed)
    rows = {"pos": (np.cumsum(rng.integers(0, gap, size=n)) + lo).astype(np.uint32),
            "strand": np.frombuffer(b"+-.", dtype=np.uint8)[rng.integers(0, 3, size=n)],
            "code_repr": np.array([modkit_amd.code_repr(codes[k]) for k in rng.integers(0, len(codes), size=n)], dtype=np.uint32)}
    for k, f in enumerate(model.COUNTS):
        rows[f] = rng.integers(0, 40 + k, size=n).astype(np.uint32)
    return rows


def rows_of(records):
    """row arrays of [(pos, code text, strand, [8 counts]), ...]"""
    rows = {"pos": np.array([r[0] for r in records], dtype=np.uint32), "strand": np.array([ord(r[2]) for r in records], dtype=np.uint8),
            "code_repr": np.array([modkit_amd.code_repr(r[1]) for r in records], dtype=np.uint32)}
    for k, f in enumerate(model.COUNTS):
        rows[f] = np.array([r[3][k] for r in records], dtype=np.uint32)
    return rows


def merged_on_device(ctx, adds, lengths):
    """adds = [(tid, rows), ...] in order -> ({tid: rows}, dropped)"""
    ctx.merge_begin(lengths)
    for tid, rows in adds:
        ctx.merge_add_rows(tid, rows)
    out, dropped = {}, 0
    for tid in range(len(lengths)):
        out[tid], dropped = ctx.merge_get(tid)
    return out, dropped


def check(ctx, adds, lengths=(1 << 31,)):
    dev, dropped = merged_on_device(ctx, adds, list(lengths))
    want_dropped = 0
    for tid in range(len(lengths)):
        records = []
        for t, rows in adds:
            if t == tid:
                records += [r for r in model.records_of_rows(rows) if r[0] < lengths[tid]]
        want = model.merge_records(records)
        got = model.records_of_rows(dev[tid])
        assert got == want, (tid, len(got), len(want))
        assert (dev[tid]["motif_idx"] == -1).all()
    for t, rows in adds:
        want_dropped += len(rows["pos"]) if not 0 <= t < len(lengths) else int((rows["pos"] >= lengths[t]).sum())
    assert dropped == want_dropped
    return dev


@pytest.mark.parametrize("na", SIZES)
def test_two_sets_of_every_size(ctx, na):
    for nb in SIZES:
        a, b = make_rows(na, seed=1000 + na), make_rows(nb, seed=2000 + nb)
        check(ctx, [(0, a), (0, b)])                                                  # interleaved (and A empty / B empty)
        span = int(a["pos"][-1]) + 1 if na else 0
        check(ctx, [(0, make_rows(na, seed=1000 + na, lo=10 * T)), (0, b)])           # B wholly before A
        check(ctx, [(0, a), (0, make_rows(nb, seed=2000 + nb, lo=span))])             # B wholly behind A
    a = make_rows(na, seed=1000 + na)
    check(ctx, [(0, a), (0, a)])                                                      # identical inputs: every key joins
    check(ctx, [(0, a)])                                                              # one input: its own duplicates collapse


@pytest.mark.parametrize("run", [2, 3, 5])
def test_a_run_of_equal_keys_on_and_across_a_tile_edge(ctx, run):
    n = 2 * T + 5
    for first in range(T - run - 1, T + 2):   # the run ends before the edge, lies across it, starts on it and behind it
        recs = [(2 * i, "m", "+", [i % 7 + 1] * 8) for i in range(n)]
        for j in range(first, first + run):
            recs[j] = (2 * first, "h", "-", [j, 1, 2, 3, 4, 5, 6, 7])
        dev = check(ctx, [(0, rows_of(recs))])                                  # duplicates inside one input, into an empty table
        assert len(dev[0]["pos"]) == n - run + 1
        half = [r for k, r in enumerate(recs) if k % 2 == 0 or first <= k < first + run - 1]
        rest = [r for k, r in enumerate(recs) if not (k % 2 == 0 or first <= k < first + run - 1)]
        check(ctx, [(0, rows_of(half)), (0, rows_of(rest))])                    # the run split over both inputs


def test_strands_and_chebi_and_letter_codes_at_one_position(ctx):
    codes = ["a", "21839", "Z", "5", "m", "76"]
    recs = [(7, c, s, [3, 1, 1, 1, 0, 0, 0, 0]) for s in "-.+" for c in codes] + [(9, "m", "+", [1] * 8)]
    order = np.random.default_rng(5).permutation(len(recs) - 1)
    dev = check(ctx, [(0, rows_of([(3, "m", "-", [2] * 8)] + [recs[i] for i in order] + recs[-1:])), (0, rows_of(recs[:7]))])
    got = [(int(p), model.code_text(c), chr(s)) for p, c, s in zip(dev[0]["pos"], dev[0]["code_repr"], dev[0]["strand"])]
    # '+' < '-' < '.'; letters by code point ("5" is the letter '5'), then ChEBI numbers by number: the derived Ord that the reference's sort calls
    assert got == [(3, "m", "-")] + [(7, c, s) for s in "+-." for c in ["5", "Z", "a", "m", "76", "21839"]] + [(9, "m", "+")]


def test_twenty_distinct_codes(ctx):
    codes = [chr(ord("a") + k) for k in range(12)] + [str(17000 + 13 * k) for k in range(8)]
    a, b = make_rows(T + 9, seed=31, gap=2, codes=codes), make_rows(2 * T, seed=32, gap=2, codes=codes)
    dev = check(ctx, [(0, a), (0, b)])
    assert len(set(dev[0]["code_repr"].tolist())) == 20


# ---- 2. limits, drops, folds, fuzz, misuse
@pytest.mark.parametrize("field", ["n_valid", "n_diff"])
def test_counts_at_the_32_bit_limit(ctx, field):
    k = model.COUNTS.index(field)
    big, zero, one = [5] * 8, [0] * 8, [0] * 8
    big[k], one[k] = U32, 1
    a = [(4, "m", "+", big), (6, "m", "+", [1] * 8)]
    dev = check(ctx, [(0, rows_of(a)), (0, rows_of([(4, "m", "+", zero)]))])      # 2^32 - 1 + 0 merges exactly
    assert int(dev[0][field][0]) == U32
    ctx.merge_begin([100])
    ctx.merge_add_rows(0, rows_of(a))
    ctx.merge_add_rows(0, rows_of([(4, "m", "+", one)]))                          # 2^32 - 1 + 1 does not fit
    with pytest.raises(modkit_amd.MkpError) as e:
        ctx.merge_get(0)
    assert e.value.status == UNSUPPORTED and "32 bits" in str(e.value)
    ctx.merge_begin([100])                                                        # inside one input as well
    ctx.merge_add_rows(0, rows_of(a + [(6, "m", "+", big)]))
    with pytest.raises(modkit_amd.MkpError) as e:
        ctx.merge_get(0)
    assert e.value.status == UNSUPPORTED
    check(ctx, [(0, rows_of(a))])                                                 # a new session starts clean


def test_rows_beyond_the_contig_are_dropped_and_counted(ctx):
    a, b = make_rows(T + 50, seed=41), make_rows(300, seed=42)
    length = int(a["pos"][T])
    assert (a["pos"] >= length).sum() > 10 and (b["pos"] < length).all()
    check(ctx, [(0, a), (1, b), (2, b), (-1, b), (0, b)], lengths=(length, 1 << 20))   # tids 2 and -1 are not in the sizes
    check(ctx, [(0, a)], lengths=(0,))


def test_three_way_fold_in_every_order(ctx):
    sets = [make_rows(T + 3, seed=51), make_rows(700, seed=52, lo=100), make_rows(2 * T + 1, seed=53, gap=2)]
    first = None
    for order in itertools.permutations(range(3)):
        dev = check(ctx, [(0, sets[i]) for i in order])
        text = {f: dev[0][f].tolist() for f in FIELDS}
        first = first or text
        assert text == first


def test_seeded_fuzz_over_two_contigs(ctx):
    rng = np.random.default_rng(61)
    adds = []
    for k in range(6):
        rows = make_rows(int(rng.integers(1, 1500)), seed=600 + k, lo=int(rng.integers(0, 400)), gap=int(rng.integers(1, 5)),
                         codes=("m", "h", "a", "21839", "76792"))
        adds.append((k % 2, rows))
    assert sum(len(r["pos"]) for _, r in adds) > 2000 and {t for t, _ in adds} == {0, 1}
    check(ctx, adds, lengths=(3000, 1200))


def test_misuse(tmp_path):
    ctx = modkit_amd.Context()
    try:
        rows = make_rows(10, seed=71, gap=5)
        for call in (lambda: ctx.merge_add_rows(0, rows), ctx.merge_add_resident, lambda: ctx.merge_get(0)):   # before merge_begin
            with pytest.raises(modkit_amd.MkpError) as e:
                call()
            assert e.value.status == INVALID and "mkp_merge_begin" in str(e.value)
        ctx.merge_begin([1000])
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.merge_add_rows(0, {f: v[::-1].copy() for f, v in rows.items()})
        assert e.value.status == INVALID and "ascending" in str(e.value)
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.merge_add_resident()                                   # nothing is resident
        assert e.value.status == INVALID
        ctx.set_partition_tags(["HP"])
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.merge_add_resident()
        assert e.value.status == INVALID and "partition" in str(e.value)
        ctx.set_partition_tags([])
        ctx.pileup_hemi_run([os.path.join(FIX, "duplex_modcalls_sort.bam"), "-o", str(tmp_path / "hemi.bed"), "--motif", "CG", "0", "--region",
                             "chr20:22,613,835-22,640,468", "--no-filtering", "-r", hemi_reference_fasta(tmp_path)])
        with pytest.raises(modkit_amd.MkpError) as e:
            ctx.merge_add_resident()                                   # pileup-hemi rows are pattern counts
        assert e.value.status == INVALID and "hemi" in str(e.value)
    finally:
        ctx.close()


# ---- 3. fused runs and the stand-alone subcommand
HG_FLAGS = ["--no-filtering", "--force-allow-implicit", "--region", "chr20:60000-170000", "--shard-bp", "30000", "-i", "10000"]
FUSED = {
    "nofilt": (BC, ["-i", "25", "--no-filtering", "--only-tabs"], {}),                                      # event pipeline
    "nofilt_host_ingest": (BC, ["-i", "25", "--no-filtering", "--only-tabs", "--host-ingest"], {}),
    "cpg": (BC, ["--no-filtering", "--cpg", "--ref", REF], {}),                                              # slot pipeline, fused decoder
    "cpg_unfused_decoder": (BC, ["--no-filtering", "--cpg", "--ref", REF], {"MKP_FUSED": "0"}),
    "two_motifs": (BC, ["--no-filtering", "--motif", "CG", "0", "--motif", "C", "0", "--ref", REF], {}),  # the rows of a position collapse
    "region": (BC, ["--no-filtering", "--region", "oligo_1512_adapters:20-60"], {}),                         # prior rows outside it still come out
    "hg002_shards": (HG, HG_FLAGS + ["--hbm-budget-mb", "1"], {}),                                           # several shards on one contig
    "hg002_shards_host_ingest": (HG, HG_FLAGS + ["--host-ingest"], {}),
    "bgzf": (BC, ["--no-filtering", "--bgzf"], {}),
}


def bam_sizes(path):
    """`name<tab>length` per contig of a BAM header (SAM spec 4.2), as a genome-sizes text"""
    with gzip.open(path, "rb") as f:
        assert f.read(4) == b"BAM\x01"
        f.read(struct.unpack("<i", f.read(4))[0])
        out = []
        for _ in range(struct.unpack("<i", f.read(4))[0]):
            name = f.read(struct.unpack("<i", f.read(4))[0])[:-1].decode()
            out.append("%s\t%d\n" % (name, struct.unpack("<i", f.read(4))[0]))
    return "".join(out)


def run_with_env(env, fn, *args):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn(*args)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def prior_tables(tmp_path, plain_text, sizes_text):
    """two prior tables cut from the run's own plain output: every third line with other counts (keys that join), lines moved by one
    position (keys that do not, also across the shard seams), a line beyond its contig, one on an unlisted contig, a '#' line, two names on
    one key; and a table with a row without coverage on every contig of the header"""
    lines = plain_text.splitlines()
    sizes = [l.split() for l in sizes_text.splitlines()]
    p1 = ["#a prior table"]
    for k, l in enumerate(lines):
        f = l.split()
        if k % 3 == 0:
            p1.append("\t".join(f[:4] + ["7"] + f[5:9] + ["7", "0.00", "3", "2", "1", "0", "1", "2", "5"]))
        if k % 5 == 0:
            p1.append("\t".join([f[0], str(int(f[1]) + 1), str(int(f[1]) + 2), f[3].split(",")[0] + ",CG,0"] + f[4:6] + [str(int(f[1]) + 1), str(int(f[1]) + 2)] + f[8:]))
            p1.append("\t".join([f[0], str(int(f[1]) + 1), str(int(f[1]) + 2), f[3].split(",")[0] + ",CGCG,2"] + f[4:6] + [str(int(f[1]) + 1), str(int(f[1]) + 2)] + f[8:]))
    p1.sort(key=lambda l: (l.split()[0], int(l.split()[1])) if not l.startswith("#") else ("", 0))
    p1.append("\t".join([sizes[0][0], sizes[0][1], str(int(sizes[0][1]) + 1), "m", "4", "+", sizes[0][1], str(int(sizes[0][1]) + 1), "255,0,0", "4", "50.00", "2", "2", "0", "0", "0", "0", "0"]))
    p1.append("no_such_contig\t5\t6\tm\t4\t+\t5\t6\t255,0,0\t4\t50.00\t2\t2\t0\t0\t0\t0\t0")
    p2 = ["\t".join([name, "3", "4", "21839", "0", ".", "3", "4", "255,0,0", "0", "0.00", "0", "0", "0", "0", "0", "0", "9"]) for name, _ in sizes]
    a, b = tmp_path / "prior1.bed", tmp_path / "prior2.bed"
    a.write_text("\n".join(p1) + "\n"); b.write_text("\n".join(p2) + "\n")
    return [str(a), str(b)]


@pytest.mark.parametrize("case", sorted(FUSED))
def test_fused_output_is_the_models_merge_of_the_plain_output_with_the_priors(tmp_path, case):
    bam, flags, env = FUSED[case]
    sizes = bam_sizes(bam)
    plain, merged = str(tmp_path / "plain.bed"), str(tmp_path / "merged.bed")
    run_with_env(env, modkit_amd.pileup, [bam, plain] + [f for f in flags if f != "--bgzf"])
    plain_text = open(plain).read()
    priors = prior_tables(tmp_path, plain_text, sizes)
    c = modkit_amd.Context()
    try:
        rep = run_with_env(env, c.pileup_run, [bam, merged] + flags + [x for p in priors for x in ("--merge-bedmethyl", p)])
    finally:
        c.close()
    want, dropped = model.merge_texts([plain_text] + [open(p).read() for p in priors], sizes)
    got = gzip.open(merged, "rb").read().decode() if case == "bgzf" else open(merged).read()
    assert got == want
    assert dropped == 2 and rep.n_rows == len(want.splitlines()) > len(plain_text.splitlines()) > 0
    assert "\tNaN\t" in want                                   # the 21839 rows of the second prior have no valid coverage
    if case.startswith("hg002"):
        assert rep.n_shards > 1
    if case == "two_motifs":
        assert any("," in l.split()[3] for l in plain_text.splitlines()) and not any("," in l.split("\t")[3] for l in want.splitlines())
        keys = [tuple(l.split()[i] for i in (0, 1, 5)) + (l.split()[3].split(",")[0],) for l in plain_text.splitlines()]
        assert len(set(keys)) < len(keys)                      # the plain run has two rows on one key
    if case == "region":
        assert any(not 20 <= int(l.split()[1]) < 60 for l in want.splitlines() if l.startswith("oligo_1512_adapters"))
    if case == "bgzf":
        assert os.path.exists(merged + ".tbi")


def test_stand_alone_subcommand_on_three_files(tmp_path):
    sizes_text = "oligo_741_adapters\t741\noligo_1512_adapters\t80\nunused\t9\n"
    a = open(os.path.join(FIX, "modbam.modpileup_nofilt.methyl.bed")).read()
    b = open(os.path.join(FIX, "modbam.modpileup_filt025.methyl.bed")).read()
    c = open(os.path.join(FIX, "cgcg2_cg0_test1.bed")).read() + "oligo_741_adapters 700 701 21839 0 . 700 701 255,0,0 0 0.00 0 0 0 0 0 0 4\n"
    paths = []
    for name, text in (("a.bed", a), ("b.bed", b), ("c.bed", c)):
        (tmp_path / name).write_text(text); paths.append(str(tmp_path / name))
    sizes = tmp_path / "g.sizes"; sizes.write_text(sizes_text)
    out = str(tmp_path / "out.bed")
    want, want_dropped = model.merge_texts([a, b, c], sizes_text)
    assert want_dropped > 0 and "\tNaN\t" in want and want.startswith("oligo_741_adapters\t")
    assert modkit_amd.bedmethyl_merge(paths + ["-g", str(sizes), "-o", out]) == (len(want.splitlines()), want_dropped)
    assert open(out).read() == want
    with pytest.raises(modkit_amd.MkpError) as e:                # the output exists now
        modkit_amd.bedmethyl_merge(paths + ["-g", str(sizes), "-o", out])
    assert e.value.status == IO
    assert modkit_amd.bedmethyl_merge(paths[::-1] + ["-g", str(sizes), "-o", out, "--force", "--bgzf"]) == (len(want.splitlines()), want_dropped)
    assert gzip.open(out, "rb").read().decode() == want and os.path.exists(out + ".tbi")
    # the reference's own test property: a file merged with itself keeps its lines and doubles its counts
    twice = str(tmp_path / "twice.bed")
    n, dropped = modkit_amd.bedmethyl_merge([paths[0], paths[0], "-g", str(sizes), "-o", twice])
    kept = [l for l in a.splitlines() if int(l.split()[1]) < 80]
    assert (n, dropped) == (len(kept), 2 * (len(a.splitlines()) - len(kept)))
    for la, lb in zip(kept, open(twice).read().splitlines()):
        fa, fb = la.split(), lb.split()
        assert fa[:4] == fb[:4] and fa[5:9] == fb[5:9] and fa[10] == fb[10]
        assert [2 * int(x) for x in [fa[4], fa[9]] + fa[11:]] == [int(x) for x in [fb[4], fb[9]] + fb[11:]]


# ---- 4. refusals
def test_refusals(tmp_path):
    prior = tmp_path / "p.bed"; prior.write_text(open(os.path.join(FIX, "modbam.modpileup_nofilt.methyl.bed")).read())
    mb = ["--merge-bedmethyl", str(prior)]
    def refused(argv, status, word, run=modkit_amd.pileup):
        with pytest.raises(modkit_amd.MkpError) as e:
            run(argv)
        assert e.value.status == status and word in str(e.value), (argv, str(e.value))
    base = [BC, str(tmp_path / "x.bed"), "--no-filtering"]
    refused([BC, str(tmp_path / "parts"), "--no-filtering", "--partition-tag", "HP"] + mb, INVALID, "--partition-tag")
    refused(base + ["--bedgraph"] + mb, INVALID, "--bedgraph")
    refused(base + ["--region-stats", str(prior), "--region-stats-out", str(tmp_path / "t.tsv")] + mb, INVALID, "--region-stats")
    refused(base + ["--localize", str(prior), "--localize-out", str(tmp_path / "t.tsv")] + mb, INVALID, "--localize")
    refused(base + ["--plan-only"] + mb, INVALID, "--plan-only")
    refused(base + ["--gpus-world", "2", "--gpus-rank", "0"] + mb, UNSUPPORTED, "--gpus-world")
    refused([os.path.join(FIX, "duplex_modcalls_sort.bam"), "-o", str(tmp_path / "h.bed"), "--cpg", "--ref", REF] + mb, INVALID,
            "unexpected argument '--merge-bedmethyl'", run=modkit_amd.pileup_hemi)
    # a prior table that does not parse, and a compressed one, fail the run
    bad = tmp_path / "bad.bed"; bad.write_text("oligo_1512_adapters\t1\t2\tm\n")
    refused(base + ["--merge-bedmethyl", str(bad)], IO, "line 1 of")
    gz = tmp_path / "p.bed.gz"; gz.write_bytes(gzip.compress(prior.read_bytes()))
    refused(base + ["--merge-bedmethyl", str(gz)], UNSUPPORTED, "plain text")
