"""What the dmr replicates tests share: seeded table sets, a session through add_rows, and the comparison of a device result (or a table
text) with the model of tests/dmr_reps_model.py.

Tolerances are dmr_sites_cases': integers, text layout, pct_*, effect sizes and p-values of exactly 0, 1 or NaN are exact (an effect size is
exact only if the balanced counts behind it are); the score keeps dmr pair's bound; every p-value (collapsed, balanced, each replicate
pair) is within the sum of the bounds of its ln_effect and ln_null, 4 * 2^-52 * S each.  In a seeded set a site with an evaluation whose
branch could flip between libms (dmr_sites_model.flippable) is left out whole; SEEDS are chosen so that a set leaves out at most 1 % of
its evaluations and 3 % of its sites (test_dmr_reps_host.py checks that with the model alone)."""
import random

import dmr_reps_model as model
import dmr_sites_model as sites_model
from dmr_pair_cases import code_repr, rows_of, score_tolerance
from dmr_sites_cases import UNIT, by_chrom, check_pvalue, model_dict

SEEDS = list(range(30))
CAP_EVALUATIONS, CAP_SITES = 0.01, 0.03


def site(chrom, pos, nv, mods, strand="+", n_can=None):
    """the rows of one position: mods = {code: n_mod}"""
    nc = nv - sum(mods.values()) if n_can is None else n_can
    return [(chrom, pos, code, strand, nv, nm, nc) for code, nm in mods.items()]


def fuzz_tables(seed):
    """2 - 4 tables a side over two contigs: a position is held by a random subset of the samples; now and then an inconsistent position"""
    rng = random.Random(1000 + seed)
    fasta = {c: "".join(rng.choice("ACGTCG") for _ in range(rng.randint(300, 500))) for c in ("k1", "k2")}
    n = [rng.randint(2, 4), rng.randint(2, 4)]
    if seed % 3 == 0:
        n[1] = n[0]   # matched
    tables = [[[] for _t in range(n[s])] for s in range(2)]
    for c, seq in fasta.items():
        for p, base in enumerate(seq):
            if base not in "CG":
                continue
            for s in range(2):
                for t in range(n[s]):
                    if rng.random() < 0.3:
                        continue
                    nv = rng.randint(0, 200) if rng.random() < 0.2 else rng.randint(1, 40)
                    codes = rng.choice([["m"], ["m"], ["h", "m"], ["h", "m", "21839"], ["h"]])
                    left, mods = nv, {}
                    for code in codes:
                        mods[code] = rng.randint(0, left)
                        left -= mods[code]
                    group = site(c, p, nv, mods, strand="+" if base == "C" else "-")
                    if rng.random() < 0.0004:   # an inconsistent position
                        x = list(group[0])
                        x[6] += 1
                        group[0] = tuple(x)
                    tables[s][t] += group
    return tables[0], tables[1], fasta


def left_out_of(res):
    """[sites left out, sites, evaluations that could flip, evaluations] of a model result"""
    out = [0, 0, 0, 0]
    for s in res["sites"]:
        evs = model.evaluations(s)
        flips = sum(1 for e in evs if sites_model.flippable(e))
        out[0] += flips > 0
        out[1] += 1
        out[2] += flips
        out[3] += len(evs)
    return out


def session(ctx, tables_a, tables_b, fasta, names=None, cut=None, order=None, lookup=None, **kw):
    """One dmr replicates session through add_rows.  names = the tids' contig names (default: every name in sight, sorted); cut = {(side,
    replicate, chrom): [row indices]} adds a contig in pieces; order = a function sorting the (side, replicate, chrom, piece) add calls (a
    contig's pieces of one table must stay ascending).  Returns (dmr_reps_get's dict, names)."""
    import modkit_amd
    if names is None:
        names = sorted(set(fasta) | {r[0] for t in list(tables_a) + list(tables_b) for r in t})
    lk = None
    if lookup is not None:
        lk = modkit_amd.dmr_default_lookup()
        lk.update({code_repr(c): b for c, b in lookup.items() if c not in model.sites.DEFAULT_LOOKUP})
    ctx.dmr_reps_begin(names, len(tables_a), len(tables_b), lookup=lk, **kw)
    for c, seq in fasta.items():
        ctx.dmr_reps_set_reference(names.index(c), seq)
    calls = []
    for side, tables in enumerate((tables_a, tables_b)):
        for rep, recs in enumerate(tables):
            for c, rs in by_chrom(recs).items():
                edges = [0] + list((cut or {}).get((side, rep, c), [])) + [len(rs)]
                for k, (lo, hi) in enumerate(zip(edges, edges[1:])):
                    if hi > lo:
                        calls.append((side, rep, c, k, rs[lo:hi]))
    if order is not None:
        calls.sort(key=order)
    for side, rep, c, _k, rs in calls:
        ctx.dmr_reps_add_rows(side, rep, names.index(c), rows_of(rs))
    return ctx.dmr_reps_get(), names


def compare(d, res, names, worst=None, left_out=None):
    """Context.dmr_reps_get's dict against the model's run(): exact parts exactly, the f64 values within tolerance.  left_out (a four-entry
    list as left_out_of returns, seeded sets only): a site with an evaluation that may flip is counted there and its p-values are not
    compared."""
    codes, want = model_dict(res, names)
    dev_codes = [chr(c) if c < 1 << 31 else str(c & 0x7fffffff) for c in d["codes"].tolist()]
    assert set(codes) <= set(dev_codes), (codes, dev_codes)
    col = [dev_codes.index(c) for c in codes]
    got = []
    for i in range(len(d["pos"])):
        ha, hb = int(d["has_code"][0][i]), int(d["has_code"][1][i])
        assert not (ha | hb) & ~sum(1 << k for k in col), "a site holds a code the model's sites do not"
        got.append((int(d["tid"][i]), int(d["pos"][i]), d["strand"][i], int(d["total"][0][i]), int(d["total"][1][i]),
                    tuple(int(d["n_mod"][0][i, k]) for k in col), tuple(int(d["n_mod"][1][i, k]) for k in col),
                    sum(1 << j for j, k in enumerate(col) if (ha >> k) & 1), sum(1 << j for j, k in enumerate(col) if (hb >> k) & 1)))
    assert got == want
    assert (d["n_a"], d["n_b"]) == (res["n_a"], res["n_b"])
    assert d["max_coverages"] == tuple(res["max_coverages"]) and d["n_sampled"] == tuple(res["n_sampled"])
    assert (d["n_batches"], d["n_batches_dropped"], d["n_model_failures"]) == (res["n_batches"], res["n_batches_dropped"], res["n_model_failures"])
    is_matched = model.matched(res["n_a"], res["n_b"])
    assert (d["rep_pvalue"] is not None) == is_matched == (d["rep_effect"] is not None)
    for i, s in enumerate(res["sites"]):
        assert (int(d["pct_samples"][0][i]), int(d["pct_samples"][1][i])) == s["pct"], (s["pos"], s["pct"])
        assert int(d["n_rep"][i]) == len(s["reps"] or []), (s["pos"], s["present"])
        sc = float(d["score"][i])
        assert abs(sc - s["score"]) <= score_tolerance(s["terms"]), (s["pos"], sc, s["score"])
        if worst is not None and s["terms"]:
            worst[1] = max(worst[1], abs(sc - s["score"]) / (UNIT * s["terms"]))
        if left_out is not None:
            evs = model.evaluations(s)
            flips = sum(1 for e in evs if sites_model.flippable(e))
            left_out[1] += 1
            left_out[2] += flips
            left_out[3] += len(evs)
            if flips:
                left_out[0] += 1
                continue
        check_pvalue(float(d["map_pvalue"][i]), float(d["effect_size"][i]), s["pmap"], worst)
        check_pvalue(float(d["balanced_map_pvalue"][i]), float(d["balanced_effect_size"][i]), s["balanced"], worst)
        for r, pm in enumerate(s["reps"] or []):
            check_pvalue(float(d["rep_pvalue"][i, r]), float(d["rep_effect"][i, r]), pm, worst)


def check_table(text, res, header=False):
    """A table text against the model: the text columns byte for byte, every f64 value parsed and within tolerance"""
    n_a, n_b = res["n_a"], res["n_b"]
    lines = text.splitlines()
    if header:
        assert lines[0] + "\n" == model.header(n_a, n_b)
        lines = lines[1:]
    assert len(lines) == len(res["sites"])
    width = 16 + (4 if model.multiple(n_a, n_b) else 0) + (2 if model.matched(n_a, n_b) else 0)
    for line, s in zip(lines, res["sites"]):
        f, want = line.split("\t"), model.site_fields(s, n_a, n_b)
        assert len(f) == width == len(want)
        assert f[:4] + f[5:14] == want[:4] + want[5:14], (f, want)
        assert abs(float(f[4]) - s["score"]) <= score_tolerance(s["terms"])
        check_pvalue(float(f[14]), float(f[15]), s["pmap"])
        if model.multiple(n_a, n_b):
            check_pvalue(float(f[16]), float(f[17]), s["balanced"])
            assert f[18:20] == want[18:20]
        if model.matched(n_a, n_b):
            if not s["reps"]:
                assert f[20:22] == ["-", "-"]
            else:
                ps, es = f[20].split(","), f[21].split(",")
                assert len(ps) == len(es) == len(s["reps"])
                for p, e, pm in zip(ps, es, s["reps"]):
                    check_pvalue(float(p), float(e), pm)
