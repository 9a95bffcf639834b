"""`dmr sites` (single-site `modkit dmr pair`) on the device (mkp_dmr_sites.hip behind mkp_dmr_sites_begin / _set_reference / _add_rows /
_add_file / _get and `mkpileup dmr sites`) against the independent model of tests/dmr_sites_model.py: integers, text, the set and order of
the sites, the max coverages and the counters exactly, the three f64 columns within the tolerances of dmr_sites_cases.
1. the two lung tables, three ways; 2. edges; 3. one site per branch; 4. the batch drop; 5. the estimate; 6. seeded tables; 7. seams;
8. misuse."""
import random

import numpy as np
import pytest

import dmr_sites_model as model
import modkit_amd
from dmr_pair_cases import TABLE_A, TABLE_B, bedmethyl_text, golden_inputs, write_fasta
from dmr_sites_cases import check_table, compare, session

pytestmark = pytest.mark.gpu
worst_seen = [0.0, 0.0]   # the largest error of a p-value / a score over the session, in units of 2^-52 * S (printed by the last test)


@pytest.fixture(scope="module")
def ctx():
    c = modkit_amd.Context()
    yield c
    c.close()


def site(chrom, pos, nv, mods, strand="+", n_can=None):
    """the rows of one position: mods = {code: n_mod}"""
    nc = nv - sum(mods.values()) if n_can is None else n_can
    return [(chrom, pos, code, strand, nv, nm, nc) for code, nm in mods.items()]


def check(ctx, a, b, fasta, left_out=None, **kw):
    """one session through add_rows against the model; returns (the device's dict, the model's result)"""
    names = kw.pop("names", None)
    cut = kw.pop("cut", None)
    rename = {"min_valid_coverage": "min_cov", "n_sample_records": "n_sample", "interval_size": "interval"}
    mkw = {rename.get(k, k): v for k, v in kw.items()}
    if "lookup" in mkw:   # (the session adds its entries to MOD_CODE_TO_DNA_BASE, as --assign-code does)
        mkw["lookup"] = dict(model.DEFAULT_LOOKUP, **mkw["lookup"])
    want = model.run(a, b, fasta, **mkw)
    d, names = session(ctx, a, b, fasta, names=names, cut=cut, **kw)
    compare(d, want, names, worst_seen, left_out)
    return d, want


# ---- 1. the lung tables
def test_lung_tables_three_ways(ctx, tmp_path, monkeypatch):
    a, b, _regions, fasta = golden_inputs()
    fa = write_fasta(tmp_path / "ref.fa", fasta)
    for extra, kw in (([], {}), (["--max-coverages", "30", "30"], {"max_coverages": (30, 30)})):
        want = model.run(a, b, fasta, **kw)
        assert len(want["sites"]) > 10000
        argv = ["-a", TABLE_A, "-b", TABLE_B, "--ref", fa, "--base", "C", "-f"] + extra
        out = tmp_path / "dev.bed"
        assert modkit_amd.dmr_sites(argv + ["-o", out]) == len(want["sites"])
        texts = [out.read_text()]
        monkeypatch.setenv("MKP_HOST_BEDMETHYL", "1")
        out = tmp_path / "host.bed"
        assert modkit_amd.dmr_sites(argv + ["-o", out, "--header"]) == len(want["sites"])
        monkeypatch.delenv("MKP_HOST_BEDMETHYL")
        assert out.read_text().startswith(model.HEADER)
        texts.append(out.read_text()[len(model.HEADER):])
        d, names = session(ctx, a, b, fasta, **kw)
        compare(d, want, names, worst_seen)
        out = tmp_path / "rows.bed"
        modkit_amd.write_dmr_sites_table(d, names, out)
        texts.append(out.read_text())
        assert texts[0] == texts[1] == texts[2]
        check_table(texts[0], want)
        for line, sc, p, e in zip(texts[2].splitlines(), d["score"], d["map_pvalue"], d["effect_size"]):   # a printed value parses back
            f = line.split("\t")
            assert float(f[4]) == sc and (float(f[14]) == p or p != p) and (float(f[15]) == e or e != e)


# ---- 2. edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_joined_site_counts(ctx, n):
    fasta = {"c": "C" * 1200}
    a = [r for p in list(range(n)) + [1000] for r in site("c", p, 20, {"m": p % 7})]
    b = [r for p in list(range(n)) + [1001] for r in site("c", p, 30, {"m": p % 11})]
    d, want = check(ctx, a, b, fasta, max_coverages=(300, 300))
    assert len(d["pos"]) == n == len(want["sites"])


def ladder(positions, pair_rows, seed):
    """one row a position, but a two-code group (h then m) beginning at each row index of pair_rows"""
    rng, rows = random.Random(seed), []
    for p in positions:
        nv = rng.randint(1, 60)
        if len(rows) in pair_rows:
            h = rng.randint(0, nv)
            rows += site("c", p, nv, {"h": h, "m": rng.randint(0, nv - h)})
        else:
            rows += site("c", p, nv, {"m": rng.randint(0, nv)})
    return rows


def test_groups_across_tile_and_wave_edges(ctx):
    fasta = {"c": "C" * 800}
    a = ladder(range(0, 700), {63, 255, 256 + 255, 300}, 1)   # rows (63, 64): a wave edge; (255, 256) and (511, 512): tile edges
    b = ladder(range(3, 703), {63, 255, 256 + 255, 127}, 2)   # other positions than a's: b's edges are its own
    for rows in (a, b):
        for first in (63, 255, 511):
            assert rows[first][1] == rows[first + 1][1] != rows[first - 1][1] and rows[first + 2][1] != rows[first][1]
    d, want = check(ctx, a, b, fasta, max_coverages=(300, 300))
    assert len(want["sites"]) == 697 and d["codes"].tolist() == [ord("h"), ord("m")]
    assert any(len(s["a"][0]) != len(s["b"][0]) for s in want["sites"])   # (h + m against m alone: three categories)


def test_strands_and_contigs(ctx):
    seq = "".join("CGAT"[(p * 7 + p // 5) % 4] for p in range(300))
    pos_c, pos_g = [p for p in range(300) if seq[p] == "C"], [p for p in range(300) if seq[p] == "G"]
    def table(chrom, seed, skip):
        rng, rows = random.Random(seed), []
        for p in range(300):
            if p % 9 == skip:
                continue
            nv = rng.randint(1, 40)
            if seq[p] == "C":
                rows += site(chrom, p, nv, {"m": rng.randint(0, nv)}, strand="+." [rng.randint(0, 1)])
                if p % 4 == 0:
                    rows += site(chrom, p, nv, {"m": 1}, strand="-")         # a '-' row on a C: no part
            elif seq[p] == "G":
                rows += site(chrom, p, nv, {"m": rng.randint(0, nv)}, strand="-")
                if p % 4 == 1:
                    rows += site(chrom, p, nv, {"h": 0}, strand="+")         # a '+' row on a G: no part
            elif p % 6 == 0:
                rows += site(chrom, p, nv, {"m": 0})                           # a row on an A or a T: no part
        return rows
    assert pos_c and pos_g
    fasta = {"zz": seq, "b1": seq, "m5": seq, "only_fasta": seq, "no_b": seq}
    a = table("zz", 1, 0) + table("b1", 2, 1) + table("m5", 3, 2) + table("no_b", 4, 3) + table("no_fasta", 5, 4) + table("a_only", 6, 5)
    b = table("m5", 7, 6) + table("zz", 8, 7) + table("b1", 9, 8) + table("no_fasta", 10, 0)
    names = ["no_b", "m5", "a_only", "zz", "no_fasta", "only_fasta", "b1"]   # tids in yet another order
    d, want = check(ctx, a, b, fasta, names=names, max_coverages=(300, 300))
    assert [s["chrom"] for s in want["sites"]] == sorted(s["chrom"] for s in want["sites"])
    assert {s["chrom"] for s in want["sites"]} == {"b1", "m5", "zz"} and {"+", "-"} == set(d["strand"])
    d2, _ = check(ctx, a, b, fasta, names=names, max_coverages=(300, 300), mask=True, min_valid_coverage=12)
    assert 0 < len(d2["pos"]) < len(d["pos"])
    lower = {k: v.lower() if k == "zz" else v for k, v in fasta.items()}
    d3, _ = check(ctx, a, b, lower, names=names, max_coverages=(300, 300), mask=True)
    assert set(d3["tid"].tolist()) == {names.index("b1"), names.index("m5")}
    check(ctx, a, b, lower, names=names, max_coverages=(300, 300))
    check(ctx, a, b, fasta, names=names, max_coverages=(300, 300), bases=("C", "A"))
    check(ctx, a, b, fasta, names=names, max_coverages=(300, 300), lookup={"m": "C", "x": "C"})


# ---- 3. one site per branch, next to plain neighbours
def test_one_site_per_branch(ctx):
    fasta = {"c": "C" * 400}
    plain = lambda p: (site("c", p, 20, {"m": 5}), site("c", p, 20, {"m": 12}))
    cases = [
        (10, site("c", 10, 20, {"m": 1}), site("c", 10, 20, {"m": 2})),            # |e| == delta exactly: p = 1
        (20, site("c", 20, 10, {"m": 10}), site("c", 20, 10, {"m": 0})),           # e = 1
        (30, site("c", 30, 10, {"m": 0}), site("c", 30, 10, {"m": 10})),           # e = -1
        (40, site("c", 40, 301, {"m": 150}), site("c", 40, 450, {"m": 225})),      # beyond the max coverage on both sides
        (50, site("c", 50, 600, {"m": 1}), site("c", 50, 20, {"m": 9})),           # a round tie: 1 / 600 * 300 = 0.5 -> 1
        (60, site("c", 60, 0, {"m": 0}), site("c", 60, 20, {"m": 9})),             # total 0: NaN, written
        (70, site("c", 70, 262, {"m": 32}), site("c", 70, 139, {"m": 4})),         # the quadrature overflows: p = 0
        (80, site("c", 80, 273, {"m": 0}), site("c", 80, 17, {"m": 2})),           # p > 1, clamped
        (90, site("c", 90, 20, {"h": 4}), site("c", 90, 20, {"m": 9})),            # h alone against m alone: the model fails, not written
        (100, site("c", 100, 30, {"h": 4, "m": 9}), site("c", 100, 25, {"h": 1, "m": 20})),   # Dirichlet
        (110, site("c", 110, 300, {"m": 15}), site("c", 110, 300, {"m": 31})),     # |e| just above delta: |d| < delta, the null form twice
    ]
    a, b = [], []
    for p, ra, rb in cases:
        for q, (xa, xb) in ((p - 3, plain(p - 3)), (p + 3, plain(p + 3))):
            a += xa
            b += xb
        a += ra
        b += rb
    a.sort(key=lambda r: r[1])
    b.sort(key=lambda r: r[1])
    d, want = check(ctx, a, b, fasta, max_coverages=(300, 300))
    by_pos = {s["pos"]: s["pmap"] for s in want["sites"]}
    assert by_pos[10]["p"] == 1.0 and by_pos[10]["ln_effect"] is None and abs(by_pos[10]["effect"]) == 0.05
    assert by_pos[20]["effect"] == 1.0 and by_pos[30]["effect"] == -1.0
    assert by_pos[50]["effect"] == 1 / 300 - 9 / 20
    assert by_pos[60]["p"] != by_pos[60]["p"]
    assert by_pos[70]["p"] == 0.0 and by_pos[70]["top"] > model.EXP_OVERFLOW + 20
    assert by_pos[80]["p"] == 1.0 and by_pos[80]["ln_null"] - by_pos[80]["ln_effect"] > 1.0
    assert 90 not in by_pos and want["n_model_failures"] == 1 == d["n_model_failures"]
    assert by_pos[110]["top"] is None and by_pos[110]["ln_null"] is not None
    got = dict(zip(d["pos"].tolist(), d["map_pvalue"].tolist()))
    assert got[10] == 1.0 and got[60] != got[60] and got[70] == 0.0 and got[80] == 1.0
    # another prior, delta and smaller max coverages move every branch
    check(ctx, a, b, fasta, max_coverages=(40, 25), prior=(2.0, 0.5), delta=0.1)


# ---- 4. the batch drop
DROP_FASTA = {"c1": "C" * 130, "c2": "C" * 120}   # -i 50: c1 [0, 50), [50, 100), then [100, 130) + c2 [0, 50), c2 [50, 100), and the rest


def drop_tables():
    a = [r for c, n in (("c1", 130), ("c2", 120)) for p in range(0, n, 3) for r in site(c, p, 20, {"h": p % 5, "m": p % 7})]
    b = [r for c, n in (("c1", 130), ("c2", 120)) for p in range(0, n, 3) for r in site(c, p, 24, {"h": p % 3, "m": p % 11})]
    return a, b


@pytest.mark.parametrize("kind", ["n_valid", "n_canonical", "sum"])
@pytest.mark.parametrize("where", [(0, "c1", 51), (1, "c1", 99), (0, "c1", 61), (1, "c2", 3), (0, "c1", 102), (1, "c2", 117), (0, "c1", 0)])
def test_an_inconsistent_position_drops_its_batch(ctx, kind, where):
    sample, chrom, pos = where
    tables = list(drop_tables())
    rows = [r for r in tables[sample] if not (r[0] == chrom and r[1] == pos)]   # (61 is a position the tables do not hold: the other sample lacks it)
    c, p, _code, st, nv, _nm, nc = site(chrom, pos, 20, {"h": 2, "m": 3})[0]
    bad = {"n_valid": [(c, p, "h", st, nv, 2, nc), (c, p, "m", st, nv + 1, 3, nc)],
           "n_canonical": [(c, p, "h", st, nv, 2, nc), (c, p, "m", st, nv, 3, nc - 1)],
           "sum": [(c, p, "h", st, nv, 2, nc), (c, p, "m", st, nv, 4, nc)]}[kind]
    tables[sample] = sorted(rows + bad, key=lambda r: (r[0], r[1]))
    d, want = check(ctx, tables[0], tables[1], DROP_FASTA, max_coverages=(300, 300), interval_size=50, batch_size=2)
    assert want["n_batches"] == 5 and want["n_batches_dropped"] == 1 == d["n_batches_dropped"]
    # the neighbouring batches stay whole: 84 positions in both tables, by batch 17, 17, 10 + 17, 17 and 6
    in_batch = {("c1", 0): 17, ("c1", 51): 17, ("c1", 99): 17, ("c1", 61): 17, ("c1", 102): 27, ("c2", 3): 27, ("c2", 117): 6}[(chrom, pos)]
    assert len(d["pos"]) == 84 - in_batch


def test_no_drop_without_an_inconsistency(ctx):
    a, b = drop_tables()
    d, want = check(ctx, a, b, DROP_FASTA, max_coverages=(300, 300), interval_size=50, batch_size=2)
    assert d["n_batches"] == 5 and d["n_batches_dropped"] == 0 and len(d["pos"]) == 44 + 40


# ---- 5. the estimate
def cov_rows(positions, seed, top=60):
    rng = random.Random(seed)
    return [r for p in positions for r in site("c", p, rng.randint(1, top), {"m": 0})]


@pytest.mark.parametrize("b_positions, sampled", [
    (list(range(0, 400, 2)), (100, 50)),                               # both reach 10 in the first super-batch
    ([3, 40, 77, 98] + list(range(100, 400, 2)), (200, 54)),           # b reaches it a super-batch later than a
    ([3, 40, 150, 180, 250, 310, 390], (400, 7)),                      # b never does: the walk runs to its end
])
def test_estimate_stops_behind_the_right_super_batch(ctx, b_positions, sampled):
    fasta = {"c": "C" * 400}   # -i 50, --batch-size 2: a super-batch is 100 bp
    a, b = cov_rows(range(400), 1), cov_rows(b_positions, 2)
    d, want = check(ctx, a, b, fasta, n_sample_records=10, interval_size=50, batch_size=2)
    assert want["n_sampled"] == sampled == d["n_sampled"] and d["max_coverages"] == want["max_coverages"]


def test_estimate_rows_not_sites_and_the_cap(ctx):
    fasta = {"c": "C" * 400}
    a = [r for p in range(0, 400, 2) for r in site("c", p, 350 + p % 90, {"h": 1, "m": 2})]   # two rows a position count twice
    b = cov_rows(range(0, 400, 2), 3, top=500)
    d, want = check(ctx, a, b, fasta, n_sample_records=60, interval_size=50, batch_size=1)
    assert d["n_sampled"] == (150, 75) and d["max_coverages"][0] == 300 and want["max_coverages"] == d["max_coverages"]
    one = cov_rows([7], 4)
    with pytest.raises(model.ModelError):
        model.run(a, one, fasta, n_sample=60, interval=50, batch_size=1)
    with pytest.raises(modkit_amd.MkpError) as e:
        session(ctx, a, one, fasta, n_sample_records=60, interval_size=50, batch_size=1)
    assert e.value.status == -1 and "percentile" in str(e.value)
    d, _ = check(ctx, a, one, fasta, max_coverages=(1000, 2), interval_size=50, batch_size=1)
    assert d["max_coverages"] == (300, 2) and d["n_sampled"] == (0, 0)


# ---- 6. seeded tables
def fuzz_tables(seed):
    rng = random.Random(seed)
    fasta = {c: "".join(rng.choice("ACGTCG") for _ in range(rng.randint(600, 1000))) for c in ("k1", "k2")}
    tables = []
    for _s in range(2):
        rows = []
        for c, seq in fasta.items():
            for p, base in enumerate(seq):
                if base not in "CG" or rng.random() < 0.15:
                    continue
                nv = rng.randint(0, 400) if rng.random() < 0.3 else rng.randint(1, 40)
                codes = rng.choice([["m"], ["m"], ["h", "m"], ["h", "m", "21839"], ["h"]])
                left, mods = nv, {}
                for code in codes:
                    mods[code] = rng.randint(0, left)
                    left -= mods[code]
                group = site(c, p, nv, mods, strand="+" if base == "C" else "-")
                if rng.random() < 0.0005:   # an inconsistent position
                    x = list(group[0])
                    x[6] += 1
                    group[0] = tuple(x)
                rows += group
        tables.append(rows)
    return tables[0], tables[1], fasta


def test_seeded_tables(ctx):
    left_out, dropped, failures = [0, 0], 0, 0
    for seed in range(50):
        a, b, fasta = fuzz_tables(seed)
        d, want = check(ctx, a, b, fasta, left_out=left_out, n_sample_records=300, interval_size=200, batch_size=2)
        dropped += want["n_batches_dropped"]
        failures += want["n_model_failures"]
    print("seeded tables: %d sites compared, %d left out, %d batches dropped, %d model failures" % (left_out[1], left_out[0], dropped, failures))
    assert left_out[1] > 20000 and left_out[0] * 100 <= left_out[1] and dropped > 10 and failures > 10


# ---- 7. seams
def test_pieces_cut_between_and_inside_positions(ctx, tmp_path, monkeypatch):
    a, b, fasta = fuzz_tables(1001)
    whole, want = check(ctx, a, b, fasta, max_coverages=(60, 60))
    k1 = [r for r in a if r[0] == "k1"]
    inside = next(i for i in range(200, len(k1)) if k1[i][1] == k1[i - 1][1])
    between = next(i for i in range(400, len(k1)) if k1[i][1] != k1[i - 1][1])
    assert 1 < inside < between
    cut, _ = check(ctx, a, b, fasta, max_coverages=(60, 60), cut={(0, "k1"): [1, inside, between], (1, "k2"): [5, 6, 7]})
    again = ctx.dmr_sites_get()   # the same session once more
    for d in (cut, again):
        for k in ("pos", "tid", "score", "map_pvalue", "effect_size"):
            assert np.array_equal(d[k], whole[k], equal_nan=True)
        assert all(np.array_equal(d[k][s], whole[k][s]) for k in ("total", "n_mod", "has_code") for s in range(2))


def test_a_table_of_several_reader_pieces(ctx, tmp_path, monkeypatch):
    rng = random.Random(5)
    fasta = {"c": "C" * 6000}
    tables = []
    for _s in range(2):
        rows = []
        for p in range(6000):
            nv = rng.randint(1, 50)
            h = rng.randint(0, nv)
            rows += site("c", p, nv, {"h": h, "m": rng.randint(0, nv - h)} if p % 3 else {"m": rng.randint(0, nv)})
        tables.append(rows)
    a, b = tables
    files = []
    for k, rows in enumerate(tables):
        text = bedmethyl_text(rows)
        assert len(text) > 4 * 65536
        files.append(tmp_path / ("t%d.bed" % k))
        files[-1].write_text(text)
    fa = write_fasta(tmp_path / "ref.fa", fasta)
    want = model.run(a, b, fasta, max_coverages=(40, 40), interval=1000, batch_size=2)
    monkeypatch.setenv("MKP_BEDMETHYL_PIECE_KB", "64")
    out = tmp_path / "out.bed"
    n = modkit_amd.dmr_sites(["-a", files[0], "-b", files[1], "--ref", fa, "--base", "C", "-o", out, "--max-coverages", "40", "40", "-i", "1000",
                              "--batch-size", "2", "--cap-coverages"])
    assert n == len(want["sites"]) == 6000
    check_table(out.read_text(), want)
    # the same files through Context.dmr_sites_add_file, with a name the tables do not hold in front
    ctx.dmr_sites_begin(["other", "c"], max_coverages=(40, 40), interval_size=1000, batch_size=2)
    ctx.dmr_sites_set_reference(1, fasta["c"])
    assert [ctx.dmr_sites_add_file(k, files[k]) for k in range(2)] == [len(a), len(b)]
    compare(ctx.dmr_sites_get(), want, ["other", "c"], worst_seen)


# ---- 8. misuse
def test_misuse_and_the_largest_errors(ctx):
    c = modkit_amd.Context()
    try:
        fasta = {"c": "C" * 50}
        a = [r for p in range(10) for r in site("c", p, 9, {"m": 3})]
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_sites_get()
        assert "mkp_dmr_sites_begin first" in str(e.value)
        c.dmr_sites_begin(["c"], max_coverages=(30, 30))
        c.dmr_sites_set_reference(0, fasta["c"])
        from dmr_pair_cases import rows_of
        c.dmr_sites_add_rows(0, 0, rows_of(a))
        with pytest.raises(modkit_amd.MkpError) as e:   # sample b has brought nothing
            c.dmr_sites_get()
        assert e.value.status == -1 and "need at least 1 contig" in str(e.value)
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_sites_add_rows(1, 3, rows_of(a))
        assert e.value.status == -1 and "unknown tid" in str(e.value)
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_sites_add_rows(2, 0, rows_of(a))
        assert e.value.status == -1
        c.dmr_sites_add_rows(1, 0, rows_of(a[5:]))
        with pytest.raises(modkit_amd.MkpError) as e:   # a piece in front of the last one
            c.dmr_sites_add_rows(1, 0, rows_of(a[:3]))
        assert e.value.status == -1 and "ascending" in str(e.value)
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_sites_add_rows(1, 0, rows_of(a[::-1]))
        assert e.value.status == -1 and "ascending" in str(e.value)
        d = c.dmr_sites_get()   # the session is still good
        assert d["pos"].tolist() == [5, 6, 7, 8, 9]
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_sites_begin(["c"], prior=(0.3, 0.3))
        assert e.value.status == -1 and "alpha + beta" in str(e.value)
    finally:
        c.close()
    print("largest error seen on the device, in units of 2^-52 * S: p-value %.3f, score %.3f (4 allowed)" % tuple(worst_seen))
