"""What the dmr sites tests share: seeded count pairs, the tolerances, the comparison of a device result (or a table text) with the model
of tests/dmr_sites_model.py, and a session through add_rows.

Tolerances.  Integers, text and f32 columns, the set and order of the written sites, the max coverages and the counters are exact.  The
score keeps dmr pair's bound: 4 * 2^-52 * sum|lgamma terms|.  ln_effect and ln_null are each allowed 4 units of 2^-52 * S, S as the model
returns it (every |lgamma value|, the two power terms, |ln of the integral| and the largest exponent inside the quadrature): the f64 model
itself stays within 0.87 of that unit of a 60-digit evaluation, and the factor 4 leaves room for another libm and another summation order,
as for the score.  map_pvalue is checked as |ln p - ln p_model| <= the sum of the two bounds; p of exactly 1 (shortcut or clamp), 0
(overflow) and NaN are exact.  effect_size is exact: two correctly rounded divisions and one subtraction."""
import math
import random

import numpy as np

import dmr_sites_model as model
from dmr_pair_cases import code_repr, rows_of, score_tolerance

FACTOR = 4.0
UNIT = 2.0 ** -52


def seeded_pairs(seed, n, max_cov=300):
    """(a_mod, a_cov, b_mod, b_cov): coverages 1 .. max_cov, fractions spread over [0, 1] with a share of extremes"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        pair = []
        for _s in range(2):
            cov = rng.randint(1, max_cov) if rng.random() < 0.7 else rng.randint(1, 30)
            f = rng.choice([0.0, 1.0, rng.random(), rng.random(), rng.random()])
            pair += [min(cov, int(round(f * cov))), cov]
        out.append(tuple(pair))
    return out


def same_float(x, y):
    return (x != x and y != y) or x == y


def check_pvalue(got_p, got_effect, pm, worst=None, got_ln=None):
    """One site's p-value and effect against the model's pmap dict; got_ln = (ln_effect, ln_null) where the caller has them"""
    assert same_float(got_effect, pm["effect"]), (got_effect, pm["effect"])
    bound = FACTOR * UNIT * (pm["s_effect"] + pm["s_null"])
    p = pm["p"]
    if got_ln is not None:
        for g, key, s in ((got_ln[0], "ln_effect", "s_effect"), (got_ln[1], "ln_null", "s_null")):
            want = pm[key]
            if want is None:
                assert g != g, (key, g)
            elif not math.isfinite(want):
                assert same_float(g, want), (key, g, want)
            else:
                assert abs(g - want) <= FACTOR * UNIT * pm[s], (key, g, want, abs(g - want) / (UNIT * pm[s]))
                if worst is not None and pm[s]:
                    worst[0] = max(worst[0], abs(g - want) / (UNIT * pm[s]))
    if p != p or p == 0.0 or pm["ln_null"] is None:
        assert same_float(got_p, p), (got_p, p)
    elif p == 1.0:
        assert got_p == 1.0, (got_p, p)   # (the clamp)
    else:
        assert got_p > 0.0 and abs(math.log(got_p) - (pm["ln_null"] - pm["ln_effect"])) <= bound, (got_p, p, bound)
        if worst is not None and bound:
            worst[0] = max(worst[0], FACTOR * abs(math.log(got_p) - (pm["ln_null"] - pm["ln_effect"])) / bound)


def model_dict(res, names):
    """The model's result as the exact parts of Context.dmr_sites_get's dict"""
    codes = sorted({c for s in res["sites"] for k in ("a", "b") for c in s[k][0]}, key=lambda c: code_repr(c))
    return codes, [(names.index(s["chrom"]), s["pos"], s["strand"], s["a"][1], s["b"][1],
                    tuple(s["a"][0].get(c, 0) for c in codes), tuple(s["b"][0].get(c, 0) for c in codes),
                    sum(1 << k for k, c in enumerate(codes) if c in s["a"][0]), sum(1 << k for k, c in enumerate(codes) if c in s["b"][0]))
                   for s in res["sites"]]


def compare(d, res, names, worst=None, left_out=None):
    """Context.dmr_sites_get's dict against the model's run(): exact parts exactly, the three f64 columns within tolerance.  left_out (a
    two-entry list, seeded tables only): a site whose branch may flip between libms (model.flippable) is counted there, [flippable, all],
    and its p-value is not compared."""
    codes, want = model_dict(res, names)
    # (the device's columns are the codes of every participating row, the model's those of the written sites: compare by code)
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
    assert d["max_coverages"] == tuple(res["max_coverages"]) and d["n_sampled"] == tuple(res["n_sampled"])
    assert (d["n_batches"], d["n_batches_dropped"], d["n_model_failures"]) == (res["n_batches"], res["n_batches_dropped"], res["n_model_failures"])
    for i, s in enumerate(res["sites"]):
        sc = float(d["score"][i])
        assert abs(sc - s["score"]) <= score_tolerance(s["terms"]), (s["pos"], sc, s["score"])
        if worst is not None and s["terms"]:
            worst[1] = max(worst[1], abs(sc - s["score"]) / (UNIT * s["terms"]))
        if left_out is not None:
            left_out[1] += 1
            if model.flippable(s["pmap"]):
                left_out[0] += 1
                continue
        check_pvalue(float(d["map_pvalue"][i]), float(d["effect_size"][i]), s["pmap"], worst)


def check_table(text, res, header=False):
    """A table text against the model: 13 columns byte for byte, the three f64 columns parsed and within tolerance, no exponent"""
    lines = text.splitlines()
    if header:
        assert lines[0] + "\n" == model.HEADER
        lines = lines[1:]
    assert len(lines) == len(res["sites"])
    for line, s in zip(lines, res["sites"]):
        f, want = line.split("\t"), model.site_fields(s)
        assert len(f) == 16
        assert f[:4] + f[5:14] == want[:4] + want[5:14], (f, want)
        for k in (4, 14, 15):
            assert "e" not in f[k].lower() or f[k] in ("inf", "-inf"), f[k]
        assert abs(float(f[4]) - s["score"]) <= score_tolerance(s["terms"])
        check_pvalue(float(f[14]), float(f[15]), s["pmap"])


def by_chrom(records):
    out = {}
    for r in records:
        out.setdefault(r[0], []).append(r)
    return out


def session(ctx, recs_a, recs_b, fasta, names=None, cut=None, lookup=None, **kw):
    """One dmr sites session through add_rows; names = the tids' contig names (default: every name in sight, sorted); cut = {(sample, chrom):
    [row indices]} adds a contig in pieces cut there.  Returns (dmr_sites_get's dict, names)."""
    import modkit_amd
    if names is None:
        names = sorted(set(fasta) | {r[0] for r in recs_a} | {r[0] for r in recs_b})
    lk = None
    if lookup is not None:
        lk = modkit_amd.dmr_default_lookup()
        lk.update({code_repr(c): b for c, b in lookup.items() if c not in model.DEFAULT_LOOKUP})
    ctx.dmr_sites_begin(names, lookup=lk, **kw)
    for c, seq in fasta.items():
        ctx.dmr_sites_set_reference(names.index(c), seq)
    for sample, recs in enumerate((recs_a, recs_b)):
        for c, rs in by_chrom(recs).items():
            edges = [0] + list((cut or {}).get((sample, c), [])) + [len(rs)]
            for lo, hi in zip(edges, edges[1:]):
                if hi > lo:
                    ctx.dmr_sites_add_rows(sample, names.index(c), rows_of(rs[lo:hi]))
    return ctx.dmr_sites_get(), names
