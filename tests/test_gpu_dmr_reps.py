"""`dmr replicates` (single-site `modkit dmr pair` over several -a / -b tables) on the device (mkp_dmr_reps.hip behind mkp_dmr_reps_begin /
_set_reference / _add_rows / _add_file / _get and `mkpileup dmr replicates`) against the independent model of tests/dmr_reps_model.py:
integers, text, the set and order of the sites, the shares of samples, the max coverages and the counters exactly, every f64 value within
the tolerances of dmr_reps_cases.
1. the lung tables 1 vs 1 (byte-equal to dmr sites) and split 2 vs 2; 2. edges; 3. presence subsets and the shapes of the sides; 4. contigs;
5. the max coverage on summed counts; 6. the batch drop; 7. the estimate; 8. seams; 9. seeded sets; 10. misuse."""
import itertools
import random

import numpy as np
import pytest

import dmr_reps_model as model
import modkit_amd
from dmr_pair_cases import TABLE_A, TABLE_B, bedmethyl_text, golden_inputs, rows_of, write_fasta
from dmr_reps_cases import CAP_EVALUATIONS, CAP_SITES, SEEDS, check_table, compare, fuzz_tables, session, site

pytestmark = pytest.mark.gpu
worst_seen = [0.0, 0.0]   # the largest error of a p-value / a score over the session, in units of 2^-52 * S (printed by the last test)
RENAME = {"min_valid_coverage": "min_cov", "n_sample_records": "n_sample", "interval_size": "interval"}


@pytest.fixture(scope="module")
def ctx():
    c = modkit_amd.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def lung():
    return golden_inputs()


def check(ctx, a, b, fasta, left_out=None, **kw):
    """one session through add_rows against the model; returns (the device's dict, the model's result)"""
    names, cut, order = kw.pop("names", None), kw.pop("cut", None), kw.pop("order", None)
    want = model.run(a, b, fasta, **{RENAME.get(k, k): v for k, v in kw.items()})
    d, names = session(ctx, a, b, fasta, names=names, cut=cut, order=order, **kw)
    compare(d, want, names, worst_seen, left_out)
    return d, want


# ---- 1. the lung tables
def test_lung_one_against_one_is_dmr_sites(ctx, lung, tmp_path):
    a, b, _regions, fasta = lung
    fa = write_fasta(tmp_path / "ref.fa", fasta)
    argv = ["-a", TABLE_A, "-b", TABLE_B, "--ref", fa, "--base", "C", "-f", "--header"]
    texts = []
    for fn, out in ((modkit_amd.dmr_sites, tmp_path / "sites.bed"), (modkit_amd.dmr_replicates, tmp_path / "reps.bed")):   # (bgzip files)
        assert fn(argv + ["-o", out]) > 10000
        texts.append(out.read_bytes())
    assert texts[0] == texts[1]
    d, names = session(ctx, [a], [b], fasta)
    ctx.dmr_sites_begin(names)
    ctx.dmr_sites_set_reference(names.index("chr20"), fasta["chr20"])
    ctx.dmr_sites_add_rows(0, names.index("chr20"), rows_of(a))
    ctx.dmr_sites_add_rows(1, names.index("chr20"), rows_of(b))
    s = ctx.dmr_sites_get()
    for k in ("pos", "tid", "score", "map_pvalue", "effect_size"):
        assert d[k].tobytes() == s[k].tobytes()
    assert d["balanced_map_pvalue"].tobytes() == s["map_pvalue"].tobytes() and d["balanced_effect_size"].tobytes() == s["effect_size"].tobytes()
    assert all(np.array_equal(d[k][x], s[k][x]) for k in ("total", "n_mod", "has_code") for x in range(2))
    assert all(d[k] == s[k] for k in ("strand", "max_coverages", "n_sampled", "n_batches", "n_batches_dropped", "n_model_failures"))
    assert d["rep_pvalue"] is None and not d["n_rep"].any() and set(d["pct_samples"][0].tolist()) == {100}
    out = tmp_path / "rows.bed"
    modkit_amd.write_dmr_reps_table(d, names, out, header=True)
    assert out.read_bytes() == texts[0]


def test_lung_split_two_against_two(ctx, lung):
    """the lung tables hold one row a position: split by row parity every site is held by one table a side, and its one replicate pair, its
    balanced and its collapsed values are one evaluation"""
    a, b, _regions, fasta = lung
    d, want = check(ctx, [a[0::2], a[1::2]], [b[0::2], b[1::2]], fasta, max_coverages=(30, 30))
    assert len(want["sites"]) > 10000 and set(d["pct_samples"][0].tolist()) == {50} == set(d["pct_samples"][1].tolist()) and set(d["n_rep"].tolist()) == {1}
    assert {tuple(s["present"][0]) for s in want["sites"]} == {(0,), (1,)} == {tuple(s["present"][1]) for s in want["sites"]}
    assert d["rep_pvalue"][:, 0].tobytes() == d["map_pvalue"].tobytes() == d["balanced_map_pvalue"].tobytes()
    assert d["rep_effect"][:, 0].tobytes() == d["effect_size"].tobytes() == d["balanced_effect_size"].tobytes()


# ---- 2. edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_joined_site_counts(ctx, n):
    fasta = {"c": "C" * 1200}
    a = [[r for p in list(range(0, n, 2)) + [1000] for r in site("c", p, 20, {"m": p % 7})], [r for p in range(1, n, 2) for r in site("c", p, 9, {"m": p % 5})] +
         site("c", 1100, 3, {"m": 1})]
    b = [[r for p in list(range(n)) + [1001] for r in site("c", p, 30, {"m": p % 11})], [r for p in range(0, n, 3) for r in site("c", p, 12, {"m": p % 4})] +
         site("c", 1150, 3, {"m": 1})]
    d, want = check(ctx, a, b, fasta, max_coverages=(300, 300))
    assert len(d["pos"]) == n == len(want["sites"])


def test_a_group_across_a_tile_edge_in_one_replicate_only(ctx):
    fasta = {"c": "C" * 700}
    rng = random.Random(4)
    def table(pairs, start):
        rows = []
        for p in range(start, 600):
            nv = rng.randint(1, 60)
            h = rng.randint(0, nv)
            rows += site("c", p, nv, {"h": h, "m": rng.randint(0, nv - h)} if len(rows) in pairs else {"m": rng.randint(0, nv)})
        return rows
    a = [table({255}, 0), table({100}, 0)]   # rows (255, 256) of a's first table are one position: a tile edge inside a group
    b = [table(set(), 2), table({511}, 1)]   # b's second table: rows (511, 512)
    assert a[0][255][1] == a[0][256][1] != a[0][254][1] and a[1][255][1] != a[1][256][1] and b[1][511][1] == b[1][512][1]
    d, want = check(ctx, a, b, fasta, max_coverages=(300, 300))
    assert len(want["sites"]) > 590 and d["codes"].tolist() == [ord("h"), ord("m")]


# ---- 3. presence subsets and the shapes of the sides
def subset_tables(n_a, n_b, seed):
    """a site for every pair of non-empty subsets of the two sides' samples"""
    rng = random.Random(seed)
    subs = lambda n: [m for m in range(1, 1 << n)]
    a, b, p = [[] for _ in range(n_a)], [[] for _ in range(n_b)], 0
    for ma, mb in itertools.product(subs(n_a), subs(n_b)):
        for tables, mask in ((a, ma), (b, mb)):
            for t in range(len(tables)):
                if (mask >> t) & 1:
                    nv = rng.randint(1, 80)
                    tables[t] += site("c", p, nv, {"m": rng.randint(0, nv)})
        p += 2
    return a, b, {"c": "C" * (p + 10)}


def test_every_subset_of_three_against_three(ctx, tmp_path):
    a, b, fasta = subset_tables(3, 3, 1)
    d, want = check(ctx, a, b, fasta, max_coverages=(300, 300))
    assert len(want["sites"]) == 49 and d["rep_pvalue"].shape == (49, 3)
    assert sorted(set(d["n_rep"].tolist())) == [0, 1, 2, 3] and sorted(set(d["pct_samples"][0].tolist())) == [33, 66, 100]
    # rank pairing where the present sets differ: a {0, 2} against b {1, 2} is (a0, b1), (a2, b2)
    s = next(s for s in want["sites"] if s["present"] == ([0, 2], [1, 2]))
    rows = {(side, t): next(r for r in tables[t] if r[1] == s["pos"]) for side, tables in ((0, a), (1, b)) for t in s["present"][side]}
    assert [r["effect"] for r in s["reps"]] == [rows[0, 0][5] / rows[0, 0][4] - rows[1, 1][5] / rows[1, 1][4],
                                                 rows[0, 2][5] / rows[0, 2][4] - rows[1, 2][5] / rows[1, 2][4]]
    out = tmp_path / "t.bed"
    modkit_amd.write_dmr_reps_table(d, ["c"], out, header=True)
    check_table(out.read_text(), want, header=True)
    assert sum(1 for l in out.read_text().splitlines() if l.endswith("\t-\t-")) == sum(1 for s in want["sites"] if not s["reps"]) > 10
    # the same tables as files through the command
    fa = write_fasta(tmp_path / "ref.fa", fasta)
    argv = ["--ref", fa, "--base", "C", "--max-coverages", "300", "300", "--header", "-o", tmp_path / "cmd.bed"]
    for flag, tables in (("-a", a), ("-b", b)):
        for t, recs in enumerate(tables):
            path = tmp_path / ("%s%d.bed" % (flag[1], t))
            path.write_text(bedmethyl_text(recs))
            argv += [flag, path]
    assert modkit_amd.dmr_replicates(argv) == 49 and (tmp_path / "cmd.bed").read_text() == out.read_text()


@pytest.mark.parametrize("n_a, n_b", [(2, 3), (1, 3), (3, 1)])
def test_unmatched_sides(ctx, tmp_path, n_a, n_b):
    a, b, fasta = subset_tables(n_a, n_b, 10 * n_a + n_b)
    d, want = check(ctx, a, b, fasta, max_coverages=(300, 300))
    assert len(want["sites"]) == ((1 << n_a) - 1) * ((1 << n_b) - 1) and d["rep_pvalue"] is None and not d["n_rep"].any()
    out = tmp_path / "t.bed"
    modkit_amd.write_dmr_reps_table(d, ["c"], out, header=True)
    check_table(out.read_text(), want, header=True)
    assert len(out.read_text().splitlines()[0].split("\t")) == 20


def test_sixteen_against_sixteen(ctx):
    rng = random.Random(16)
    a, b = [[] for _ in range(16)], [[] for _ in range(16)]
    for p, (held_a, held_b) in ((3, (range(16), range(16))), (40, ([15], range(0, 16, 2))), (77, (range(1, 16), range(15)))):
        for tables, held in ((a, held_a), (b, held_b)):
            for t in held:
                nv = rng.randint(1, 50)
                tables[t] += site("c", p, nv, {"m": rng.randint(0, nv)})
    for t in range(16):   # (every table holds a row, each at a position of its own)
        a[t] += site("c", 100 + t, 5, {"m": 1})
        b[t] += site("c", 130 + t, 5, {"m": 1})
    d, want = check(ctx, a, b, {"c": "C" * 200}, max_coverages=(300, 300))
    assert d["pos"].tolist() == [3, 40, 77] and d["n_rep"].tolist() == [16, 0, 15]
    assert d["pct_samples"][0].tolist() == [100, 6, 93] and d["pct_samples"][1].tolist() == [100, 50, 93]


# ---- 4. contigs
def test_contigs_held_by_some_samples_only(ctx):
    rng = random.Random(8)
    def rows(chrom, positions):
        out = []
        for p in positions:
            nv = rng.randint(1, 40)
            out += site(chrom, p, nv, {"m": rng.randint(0, nv)})
        return out
    fasta = {c: "C" * 120 for c in ("both", "b2_only", "no_b", "no_ref_in_tables")}
    a = [rows("both", range(0, 100, 2)) + rows("b2_only", range(0, 100, 3)) + rows("no_b", range(50)) + rows("no_fasta", range(20)),
         rows("both", range(0, 100, 3)) + rows("no_b", range(0, 50, 2))]
    b = [rows("both", range(0, 100, 5)) + rows("no_fasta", range(20)),
         rows("b2_only", range(0, 100, 2)) + rows("both", range(1, 100, 2))]
    names = ["no_b", "both", "no_fasta", "no_ref_in_tables", "b2_only"]
    d, want = check(ctx, a, b, fasta, names=names, max_coverages=(300, 300))
    assert {s["chrom"] for s in want["sites"]} == {"both", "b2_only"}
    only = [s for s in want["sites"] if s["chrom"] == "b2_only"]
    assert len(only) == 17 and all(s["present"] == ([0], [1]) and len(s["reps"]) == 1 and s["pct"] == (50, 50) for s in only)


# ---- 5. the max coverage applies to the summed coverage
def test_summed_coverage_beyond_the_max_coverage(ctx):
    a = [site("c", 5, 25, {"m": 20}) + site("c", 9, 10, {"m": 1}), site("c", 5, 28, {"m": 3}), site("c", 5, 22, {"m": 11})]
    b = [site("c", 5, 29, {"m": 2}) + site("c", 9, 10, {"m": 9}), site("c", 5, 27, {"m": 25}), site("c", 5, 21, {"m": 4})]
    d, want = check(ctx, a, b, {"c": "C" * 20}, max_coverages=(30, 30), cap_coverages=True)
    s = want["sites"][0]
    assert s["a"] == ({"m": 34}, 75) and s["b"] == ({"m": 31}, 77) and s["bal_a"] == ({"m": 34}, 75) and s["bal_b"] == ({"m": 28}, 75)
    # (a: target 25: 20 + floor(2.68) + floor(12.5) = 34 of 75; b: target 25.67 -> 25 each: floor(1.77) + floor(23.77) + floor(4.89) = 28 of 75)
    # resized on the sums (34 / 75 -> 14 / 30, 31 / 77 -> 12 / 30), not per sample
    assert d["effect_size"][0] == 14 / 30 - 12 / 30 and d["rep_effect"][0].tolist() == [20 / 25 - 2 / 29, 3 / 28 - 25 / 27, 11 / 22 - 4 / 21]
    assert d["n_rep"].tolist() == [3, 1] and d["rep_effect"][1, 0] == d["effect_size"][1] == 1 / 10 - 9 / 10
    assert d["max_coverages"] == (30, 30)
    # without --cap-coverages a side's max coverage is times its tables: 90 holds both sums, and a replicate pair resizes at 90 as well
    d, want = check(ctx, a, b, {"c": "C" * 20}, max_coverages=(30, 30))
    assert d["max_coverages"] == (90, 90) and d["effect_size"][0] == 34 / 75 - 31 / 77
    d, _ = check(ctx, a, b, {"c": "C" * 20}, max_coverages=(120, 7))
    assert d["max_coverages"] == (300, 21) and d["effect_size"][0] == 34 / 75 - 8 / 21   # (31 / 77 * 21 = 8.45 -> 8)


# ---- 6. the batch drop
DROP_FASTA = {"c1": "C" * 130, "c2": "C" * 120}   # -i 50: c1 [0, 50), [50, 100), then [100, 130) + c2 [0, 50), c2 [50, 100), and the rest


def drop_tables():
    mk = lambda nv, step, ka, kb: [r for c, n in (("c1", 130), ("c2", 120)) for p in range(0, n, step) for r in site(c, p, nv, {"h": p % ka, "m": p % kb})]
    return [mk(20, 3, 5, 7), mk(22, 6, 3, 5)], [mk(24, 3, 3, 11), mk(26, 3, 4, 9), mk(18, 9, 2, 3)]


@pytest.mark.parametrize("kind", ["n_valid", "n_canonical", "sum"])
@pytest.mark.parametrize("where", [("c1", 51), ("c1", 99), ("c1", 102), ("c2", 48), ("c1", 0), ("c2", 117)])
def test_an_inconsistent_position_in_the_last_replicate_drops_its_batch(ctx, kind, where):
    """the first and the last position of a batch (c1 51 / 99) and of the batch that spans two contigs (c1 102 / c2 48), of the first and of
    the trailing batch: the inconsistency stands in the last table of b alone, the batch is gone for every sample"""
    chrom, pos = where
    a, b = drop_tables()
    rows = [r for r in b[2] if not (r[0] == chrom and r[1] == pos)]
    c, p, _code, st, nv, _nm, nc = site(chrom, pos, 18, {"h": 2, "m": 3})[0]
    bad = {"n_valid": [(c, p, "h", st, nv, 2, nc), (c, p, "m", st, nv + 1, 3, nc)],
           "n_canonical": [(c, p, "h", st, nv, 2, nc), (c, p, "m", st, nv, 3, nc - 1)],
           "sum": [(c, p, "h", st, nv, 2, nc), (c, p, "m", st, nv, 4, nc)]}[kind]
    b[2] = sorted(rows + bad, key=lambda r: (r[0], r[1]))
    d, want = check(ctx, a, b, DROP_FASTA, max_coverages=(300, 300), interval_size=50, batch_size=2)
    assert want["n_batches"] == 5 and want["n_batches_dropped"] == 1 == d["n_batches_dropped"]
    in_batch = {("c1", 0): 17, ("c1", 51): 17, ("c1", 99): 17, ("c1", 102): 27, ("c2", 48): 27, ("c2", 117): 6}[where]
    assert len(d["pos"]) == 84 - in_batch


def test_no_drop_without_an_inconsistency(ctx):
    a, b = drop_tables()
    d, _want = check(ctx, a, b, DROP_FASTA, max_coverages=(300, 300), interval_size=50, batch_size=2)
    assert d["n_batches"] == 5 and d["n_batches_dropped"] == 0 and len(d["pos"]) == 84


# ---- 7. the estimate pools a side's samples
def cov_rows(positions, seed, top=60):
    rng = random.Random(seed)
    return [r for p in positions for r in site("c", p, rng.randint(1, top), {"m": 0})]


@pytest.mark.parametrize("b_tables, sampled", [
    ([range(0, 400, 4), range(2, 400, 4)], (150, 50)),                                      # both pools reach 12 in the first super-batch
    ([[3, 40, 77], [50, 98] + list(range(100, 400, 2)), [60]], (300, 56)),                   # b's pool reaches it a super-batch later
])
def test_estimate_pools_the_replicates(ctx, b_tables, sampled):
    fasta = {"c": "C" * 400}   # -i 50, --batch-size 2: a super-batch is 100 bp
    a = [cov_rows(range(400), 1), cov_rows(range(0, 400, 2), 2, top=200)]
    b = [cov_rows(pos, 3 + k, top=30 + 100 * k) for k, pos in enumerate(b_tables)]
    d, want = check(ctx, a, b, fasta, n_sample_records=12, interval_size=50, batch_size=2)
    assert want["n_sampled"] == sampled == d["n_sampled"] and d["max_coverages"] == want["max_coverages"]
    alone = model.run(a[:1], b[:1], fasta, n_sample=2, interval=50, batch_size=2)["max_coverages"]
    assert alone != want["max_coverages"]   # (the pool, not the first table)


# ---- 8. seams
def test_pieces_and_interleaved_tables(ctx):
    a, b, fasta = fuzz_tables(1001)
    whole, want = check(ctx, a, b, fasta, max_coverages=(60, 60), interval_size=50, batch_size=2)
    k1 = [r for r in a[1] if r[0] == "k1"]
    inside = next(i for i in range(50, len(k1)) if k1[i][1] == k1[i - 1][1])
    between = next(i for i in range(inside + 5, len(k1)) if k1[i][1] != k1[i - 1][1])
    cut = {(0, 1, "k1"): [1, inside, between], (1, 0, "k2"): [5, 6, 7], (1, len(b) - 1, "k1"): [40]}
    # the add calls by piece number first, b in front of a, the last replicate first: tables interleave, a table's pieces stay ascending
    mixed, _ = check(ctx, a, b, fasta, max_coverages=(60, 60), interval_size=50, batch_size=2, cut=cut, order=lambda c: (c[3], -c[0], -c[1], c[2]))
    again = ctx.dmr_reps_get()   # the same session once more
    for d in (mixed, again):
        for k in ("pos", "tid", "score", "map_pvalue", "effect_size", "balanced_map_pvalue", "balanced_effect_size", "n_rep"):
            assert np.array_equal(d[k], whole[k], equal_nan=True)
        assert all(np.array_equal(d[k][s], whole[k][s]) for k in ("total", "n_mod", "has_code", "pct_samples") for s in range(2))
        if whole["rep_pvalue"] is not None:
            assert np.array_equal(d["rep_pvalue"], whole["rep_pvalue"], equal_nan=True)


# ---- 9. seeded sets
def test_seeded_sets(ctx):
    total = [0, 0, 0, 0]
    dropped = failures = 0
    for seed in SEEDS:
        a, b, fasta = fuzz_tables(seed)
        out = [0, 0, 0, 0]
        _d, want = check(ctx, a, b, fasta, left_out=out, n_sample_records=300, interval_size=50, batch_size=2)
        assert out[0] <= CAP_SITES * out[1] and out[2] <= CAP_EVALUATIONS * out[3], (seed, out)
        total = [x + y for x, y in zip(total, out)]
        dropped += want["n_batches_dropped"]
        failures += want["n_model_failures"]
    print("seeded sets: %d sites (%d left out), %d evaluations (%d could flip), %d batches dropped, %d model failures" %
          (total[1], total[0], total[3], total[2], dropped, failures))
    assert total[1] > 10000 and dropped > 10 and failures > 100


# ---- 10. misuse
def test_misuse_and_the_largest_errors(ctx):
    c = modkit_amd.Context()
    try:
        rows = rows_of([r for p in range(10) for r in site("c", p, 9, {"m": 3})])
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_reps_add_rows(0, 0, 0, rows)
        assert "mkp_dmr_reps_begin first" in str(e.value)
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_reps_get()
        assert "mkp_dmr_reps_begin first" in str(e.value)
        for n_a, n_b, status in ((0, 1, -1), (1, 0, -1), (17, 1, -3), (2, 17, -3)):
            with pytest.raises(modkit_amd.MkpError) as e:
                c.dmr_reps_begin(["c"], n_a, n_b)
            assert e.value.status == status
        c.dmr_reps_begin(["c"], 2, 3, max_coverages=(30, 30))
        c.dmr_reps_set_reference(0, "C" * 50)
        for side, rep in ((2, 0), (-1, 0), (0, 2), (1, 3), (0, -1)):
            with pytest.raises(modkit_amd.MkpError) as e:
                c.dmr_reps_add_rows(side, rep, 0, rows)
            assert e.value.status == -1
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_reps_add_rows(0, 0, 3, rows)
        assert e.value.status == -1 and "unknown tid" in str(e.value)
        c.dmr_reps_add_rows(0, 1, 0, rows)
        with pytest.raises(modkit_amd.MkpError) as e:   # no b table has brought a row
            c.dmr_reps_get()
        assert e.value.status == -1 and "need at least 1 contig" in str(e.value)
        c.dmr_reps_add_rows(1, 2, 0, rows_of([r for p in range(5, 10) for r in site("c", p, 9, {"m": 3})]))
        with pytest.raises(modkit_amd.MkpError) as e:   # a piece in front of the table's last one
            c.dmr_reps_add_rows(1, 2, 0, rows)
        assert e.value.status == -1 and "ascending" in str(e.value)
        c.dmr_reps_add_rows(1, 1, 0, rows)   # (another table of the side may begin anywhere)
        d = c.dmr_reps_get()   # the session is still good
        assert d["pos"].tolist() == list(range(10)) and d["pct_samples"][1].tolist() == [33] * 5 + [66] * 5 and d["rep_pvalue"] is None
    finally:
        c.close()
    print("largest error seen on the device, in units of 2^-52 * S: p-value %.3f, score %.3f (4 allowed)" % tuple(worst_seen))
