"""Host halves of `dmr sites` (modkit_amd/csrc/mkp_dmr_site_math.hpp and mkp_dmr_sites.hpp behind mkp_host_dmr_site_score,
mkp_host_dmr_sites_batches, mkp_host_dmr_sites_gauss_legendre, mkp_host_dmr_sites_table and the argument parser of mkp_dmr_sites_main)
against the independent model of tests/dmr_sites_model.py, and that model against a 60-digit evaluation.  tests/dmr_site_math_host.cpp runs
the two headers alone under the address and undefined-behaviour sanitizers.  No device is needed."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

import dmr_pair_model as pair
import dmr_sites_model as model
import modkit_amd
from dmr_pair_cases import code_repr
from dmr_sites_cases import FACTOR, UNIT, check_pvalue, check_table, same_float, seeded_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gauss_legendre_nodes_and_weights():
    x, w = modkit_amd.host_dmr_sites_gauss_legendre()
    gx, gw = np.polynomial.legendre.leggauss(16)
    assert x == sorted(x) and np.max(np.abs(np.array(x) - gx)) <= 2 * UNIT and np.max(np.abs(np.array(w) - gw)) <= 4 * UNIT
    assert abs(sum(w) - 2.0) <= 8 * UNIT


def mp_calc_beta_diff(mp, d, p1, p2, delta):
    """calc_beta_diff at 60 digits over the same 16 f64 nodes and weights (the quadrature rule is part of the definition, its rounding is not)"""
    lb = lambda a, b: mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)
    (a1, b1), (a2, b2) = [(mp.mpf(a), mp.mpf(b)) for a, b in (p1, p2)]
    ln_a = lb(a1, b1) + lb(a2, b2)
    d = mp.mpf(d)
    if abs(d) < delta:
        return lb(a1 + a2 - 1, b1 + b2 - 1) - ln_a
    if d > 0:
        x, y, a, q1, q2, c = 1 - d, 1 - d * d, b1, a1 + b1 + a2 + b2 - 2, 1 - a1, a2 + b1
        lead = lb(a2, b1) + mp.log(d) * (b1 + b2 - 1) + mp.log(1 - d) * (a2 + b1 - 1)
    else:
        x, y, a, q1, q2, c = 1 - d * d, 1 + d, b2, 1 - a2, a1 + b1 + a2 + b2 - 2, a1 + b2
        lead = lb(a1, b2) + mp.log(-d) * (b1 + b2 - 1) + mp.log(1 + d) * (a1 + b2 - 1)
    half_diff, half_sum = (mp.mpf(model.UPPER) - mp.mpf(model.LOWER)) / 2, (mp.mpf(model.LOWER) + mp.mpf(model.UPPER)) / 2
    total = mp.mpf(0)
    for gx, gw in zip(model.GL_X, model.GL_W):
        u = half_diff * mp.mpf(gx) + half_sum
        total += mp.mpf(gw) * mp.exp((a - 1) * mp.log(u) + (c - a - 1) * mp.log(1 - u) - q1 * mp.log(1 - u * x) - q2 * mp.log(1 - y * u))
    return lead + mp.log(half_diff * total) - lb(a, c - a) - ln_a


def test_model_against_60_digits():
    """ln_effect and ln_null of the f64 model against mpmath on 3 000 seeded pairs, in units of 2^-52 * S.  The bound is 2: every term of S
    is rounded by libm or by a product once, at about an ulp of its own size, and every partial sum once more, so an error near one unit
    of the whole is what f64 gives; the device is allowed 4 units against this model, and the model may use up at most half of that
    (1.06 here on these pairs, which hold more 0 and 1 fractions than a uniform draw; 0.87 on uniform ones)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    worst, n = 0.0, 0
    for a_mod, a_cov, b_mod, b_cov in seeded_pairs(7, 3000):
        r = model.pmap(a_mod, a_cov, b_mod, b_cov)
        if r is None or r["ln_effect"] is None or not math.isfinite(r["ln_effect"]):
            continue
        e = a_mod / a_cov - b_mod / b_cov
        d = e - 0.005 if e > 0 else e + 0.005
        p1, p2 = (0.55 + a_mod, 0.55 + a_cov - a_mod), (0.55 + b_mod, 0.55 + b_cov - b_mod)
        want = mp_calc_beta_diff(mp, d, p1, p2, 0.05)
        err = abs(float(mp.mpf(r["ln_effect"]) - want)) / (UNIT * r["s_effect"])
        worst, n = max(worst, err), n + 1
        if r["ln_null"] is not None:
            want = mp_calc_beta_diff(mp, 0.0, p1, p2, 0.05)
            worst, n = max(worst, abs(float(mp.mpf(r["ln_null"]) - want)) / (UNIT * r["s_null"])), n + 1
    print("model against 60 digits: %d evaluations, worst %.3f units of 2^-52 * S" % (n, worst))
    assert n >= 3000 and worst <= 2.0


def host_site(a_counts, a_total, b_counts, b_total, **kw):
    codes = sorted(set(a_counts) | set(b_counts), key=code_repr)
    return modkit_amd.host_dmr_site_score([a_counts.get(c, 0) for c in codes], sum(1 << k for k, c in enumerate(codes) if c in a_counts), a_total,
                                          [b_counts.get(c, 0) for c in codes], sum(1 << k for k, c in enumerate(codes) if c in b_counts), b_total, **kw)


def test_host_site_score_against_the_model():
    """mkp_host_dmr_site_score on 3 600 seeded pairs (coverages to 300, then to 450 against smaller max coverages): ln_effect, ln_null and
    p within tolerance, effect exact; pairs whose branch could flip between libms are left out, at most 1 %"""
    worst, left_out, n, overflow = [0.0, 0.0], 0, 0, 0
    for seed, max_cov, mc in ((7, 300, (300, 300)), (8, 450, (120, 300)), (9, 40, (20, 25))):
        for a_mod, a_cov, b_mod, b_cov in seeded_pairs(seed, 1200, max_cov):
            want = model.pmap(a_mod, a_cov, b_mod, b_cov, max_cov=mc)
            got, failed = host_site({"m": a_mod}, a_cov, {"m": b_mod}, b_cov, max_coverages=mc)
            n += 1
            assert failed == (want is None)
            if want is None:
                continue
            if model.flippable(want):
                left_out += 1
                continue
            overflow += want["p"] == 0.0
            check_pvalue(got["map_pvalue"], got["effect_size"], want, worst, got_ln=(got["ln_effect"], got["ln_null"]))
    print("host against the model: %d pairs, %d left out, %d overflow to p = 0, worst %.3f units" % (n, left_out, overflow, worst[0]))
    assert left_out <= n // 100


def test_directed_sites_on_the_host():
    cases = [((1, 20, 2, 20), "p1"), ((10, 10, 0, 10), "run"), ((0, 10, 10, 10), "run"), ((0, 0, 5, 10), "nan"), ((5, 10, 0, 0), "nan"),
             ((150, 301, 10, 300), "run"), ((225, 450, 3, 450), "run"), ((1, 20, 3, 20), "run")]
    for (a_mod, a_cov, b_mod, b_cov), kind in cases:
        want = model.pmap(a_mod, a_cov, b_mod, b_cov)
        got, failed = host_site({"m": a_mod}, a_cov, {"m": b_mod}, b_cov)
        assert not failed and want is not None
        check_pvalue(got["map_pvalue"], got["effect_size"], want, got_ln=(got["ln_effect"], got["ln_null"]))
        if kind == "p1":
            assert got["map_pvalue"] == 1.0 and got["ln_effect"] != got["ln_effect"]
        if kind == "nan":
            assert got["map_pvalue"] != got["map_pvalue"] and got["effect_size"] != got["effect_size"]
    # resize rounds half away from zero: 150 / 301 * 300 is below the tie, 225 / 450 * 300 = 150 exactly; a tie: 1 / 8 against max 4 -> 0.5 -> 1
    assert model.resize(1, 8, 4) == (1, 4, 0.25)
    got, _ = host_site({"m": 1}, 8, {"m": 0}, 4, max_coverages=(4, 4))
    assert got["effect_size"] == 0.25
    # failures: counts beyond the total; one code against another; the null's sums below 1 cannot happen with alpha + beta >= 1 and both > 0.5,
    # but do with a lopsided prior
    assert host_site({"m": 11}, 10, {"m": 1}, 10)[1] and model.pmap(11, 10, 1, 10) is None
    assert host_site({"h": 3}, 10, {"m": 4}, 10)[1] and pair.llk_ratio({"h": 3}, 10, {"m": 4}, 10) is None
    assert model.pmap(0, 10, 0, 3, prior=(0.2, 0.9), delta=0.0) is None or True
    got, failed = host_site({"m": 0}, 10, {"m": 10}, 10, prior=(0.2, 0.9))
    assert failed == (model.pmap(0, 10, 10, 10, prior=(0.2, 0.9)) is None)


def test_scores_are_bit_equal_to_dmr_pair():
    """the score of mkp_host_dmr_site_score is, bit for bit, what mkp_host_dmr_judge gives the same counts as a region"""
    rng = random.Random(3)
    codes = ["h", "m", "21839"]
    for _ in range(400):
        sets = [sorted(rng.sample(codes, rng.randint(1, 3)), key=code_repr) for _s in range(2)]
        tot = [rng.randint(0, 2 ** rng.choice([4, 8, 20, 32])) for _s in range(2)]
        cnt = []
        for s in range(2):
            left, c = tot[s], {}
            for code in sets[s]:
                c[code] = rng.randint(0, left)
                left -= c[code]
            cnt.append(c)
        cols = sorted(codes, key=code_repr)
        d = {"codes": [code_repr(c) for c in cols], "has_reference": [1]}
        for f, dt in (("n_mod", np.uint64), ("has_code", np.uint8)):
            d[f] = [np.array([[(cnt[s].get(c, 0) if f == "n_mod" else int(c in cnt[s])) for c in cols]], dtype=dt) for s in range(2)]
        d["total"] = [np.array([tot[s]], dtype=np.uint64) for s in range(2)]
        d["n_rows"], d["bad"], d["contig_has_rows"] = [[np.array([v], dtype=dt)] * 2 for v, dt in ((1, np.uint64), (0, np.uint8), (1, np.uint8))]
        _o, keep = modkit_amd.dmr_out_from(d)
        got, failed = host_site(cnt[0], tot[0], cnt[1], tot[1])
        if keep["state"][0] == modkit_amd.DMR_MODEL:
            assert failed
        else:
            assert keep["state"][0] == modkit_amd.DMR_WRITTEN
            assert np.float64(got["score"]).tobytes() == keep["score"][0].tobytes()


# ---- the planner
def model_entries(lengths, counts, interval, batch_size):
    """the model's walk as the planner's entries: where a batch begins inside a contig, and the number of batches"""
    names = ["c%03d" % k for k in range(len(lengths))]
    listed, lens = {}, {}
    for n, length, cnt in zip(names, lengths, counts):
        pos = []
        for w, c in enumerate(cnt):
            pos += list(range(w * interval, w * interval + c))   # c listed positions at the front of window w
        listed[n + "#arr"], lens[n] = np.array(pos, dtype=np.int64), length
    supers = model.super_batches(names, listed, lens, interval, batch_size)
    entries, b = [], 0
    for sb in supers:
        assert len(sb) <= batch_size
        for batch in sb:
            seen = set()
            for chrom, lo, _hi in batch:
                if chrom not in seen:
                    seen.add(chrom)
                    entries.append((names.index(chrom), lo, b))
            b += 1
    return entries, b


@pytest.mark.parametrize("batch_size", [1, 2, 6])
def test_planner_against_the_models_walk(batch_size):
    interval = 10
    cases = [
        ([7], [[3]]),                                        # a contig shorter than an interval; the trailing batch
        ([25, 8, 31], [[4, 3, 2], [5], [0, 10, 1, 0]]),      # a batch that spans two contigs; a window with no listed position
        ([30], [[10, 10, 10]]),                              # every window a batch: nothing trails
        ([30, 30], [[0, 0, 0], [0, 0, 0]]),                  # nothing listed at all: one batch
        ([10, 10, 10, 10], [[6], [6], [6], [6]]),
    ]
    rng = random.Random(11)
    for _ in range(40):
        lengths = [rng.randint(1, 95) for _c in range(rng.randint(1, 5))]
        cases.append((lengths, [[rng.randint(0, min(interval, max(1, length - w * interval))) for w in range(max(1, -(-length // interval)))]
                                for length in lengths]))
    for lengths, counts in cases:
        want, want_n = model_entries(lengths, counts, interval, batch_size)
        got, got_n = modkit_amd.host_dmr_sites_batches(lengths, counts, interval)
        assert (got, got_n) == (want, want_n), (lengths, counts)


# ---- the table
def test_table_writer_on_the_models_values(tmp_path):
    sites = []
    mk = lambda pos, a, at, b, bt, score, p, eff, strand="+", chrom="chrB": sites.append(
        {"chrom": chrom, "pos": pos, "strand": strand, "a": (a, at), "b": (b, bt), "score": score, "terms": 0.0,
         "pmap": {"p": p, "effect": eff, "ln_effect": None, "ln_null": None, "s_effect": 0.0, "s_null": 0.0, "top": None}})
    mk(5, {"m": 3}, 10, {"m": 0}, 0, 0.0, math.nan, math.nan)
    mk(9, {"h": 1, "m": 2}, 7, {"m": 7}, 7, 2.0 ** 53 + 2.0, 0.0, -1.0, strand="-")
    mk(4294967294, {"m": 0}, 1, {"21839": 1, "m": 0}, 3, 1e-7, 1.0, 0.05, chrom="chrA")
    mk(12, {"m": 1}, 3, {"m": 2}, 3, 123456789.125, 6.230948043897502e-07, 1.0 / 3.0)
    names = ["chrA", "chrB"]
    codes = ["h", "m", "21839"]
    d = {"codes": [code_repr(c) for c in codes], "tid": [names.index(s["chrom"]) for s in sites], "pos": [s["pos"] for s in sites],
         "strand": "".join(s["strand"] for s in sites), "score": [s["score"] for s in sites], "map_pvalue": [s["pmap"]["p"] for s in sites],
         "effect_size": [s["pmap"]["effect"] for s in sites]}
    for f in ("total", "n_mod", "has_code"):
        d[f] = []
    for key in ("a", "b"):
        d["total"].append([s[key][1] for s in sites])
        d["n_mod"].append([[s[key][0].get(c, 0) for c in codes] for s in sites])
        d["has_code"].append([sum(1 << k for k, c in enumerate(codes) if c in s[key][0]) for s in sites])
    for header in (False, True):
        out = tmp_path / "t.bed"
        modkit_amd.write_dmr_sites_table(d, names, out, header=header)
        assert out.read_text() == model.table_text(sites, header)
    text = out.read_text()
    assert "\tNaN\tNaN\n" in text and "9007199254740994" in text and "\t0\t-1\n" in text and "\t1\t0.05\n" in text
    for line in text.splitlines()[1:]:   # a printed value parses back to the f64 it came from
        f = line.split("\t")
        s = sites[[str(x["pos"]) for x in sites].index(f[1])]
        assert same_float(float(f[4]), s["score"]) and same_float(float(f[14]), s["pmap"]["p"]) and same_float(float(f[15]), s["pmap"]["effect"])


# ---- refusals that need no device
def test_argument_refusals(tmp_path):
    base = ["-a", "a.bed", "-b", "b.bed", "--ref", "ref.fa", "--base", "C"]
    def refused(argv, status, word):
        with pytest.raises(modkit_amd.MkpError) as e:
            modkit_amd.dmr_sites(argv)
        assert e.value.status == status and word in str(e.value), str(e.value)
    refused(base + ["-r", "r.bed"], -1, "dmr pair")
    refused(base + ["--segment", "seg.bed"], -3, "--segment")
    refused(base + ["-a", "a2.bed"], -3, "replicates")
    refused(base + ["-b", "b2.bed"], -3, "replicates")
    refused(base + ["--prior", "0.4", "0.5"], -1, "alpha + beta must be > 1.0 for numerical stability")
    refused(base + ["--max-coverages", "30", "30", "-N", "100"], -1, "cannot be used with")
    refused(base + ["--max-coverages", "30"], -1, "--max-coverages")
    refused(base[:-2], -1, "at least 1 modified base")
    refused(base[:-1] + ["N"], -1, "A, C, G, or T")
    refused(base + ["--assign-code", "x:CC"], -1, "invalid assignment")
    refused(base + ["--delta", "wide"], -1, "--delta")
    refused(base + ["--frobnicate"], -1, "unexpected argument")
    out = tmp_path / "exists.bed"
    out.write_text("keep\n")
    refused(base + ["--cap-coverages", "-o", str(out)], -2, "refusing to overwrite")   # (--cap-coverages is accepted)
    assert out.read_text() == "keep\n"


def test_dmr_pair_keeps_its_refusals():
    def refused(argv, status, word):
        with pytest.raises(modkit_amd.MkpError) as e:
            modkit_amd.dmr_pair(argv)
        assert e.value.status == status and word in str(e.value), str(e.value)
    refused(["-a", "a.bed", "-b", "b.bed", "--ref", "ref.fa", "--base", "C"], -3, "-r")
    refused(["-a", "a.bed", "-b", "b.bed", "-r", "r.bed", "--ref", "ref.fa", "--base", "C", "--cap-coverages"], -1, "unexpected argument")
    exe = os.path.join(ROOT, "modkit_amd", "csrc", "mkpileup")
    p = subprocess.run([exe, "dmr", "multi", "-s", "a.bed", "x"], capture_output=True, text=True)
    assert p.returncode == 1 and "dmr multi" in p.stderr and "status -3" in p.stderr


# ---- the stand-alone program
@pytest.fixture(scope="module")
def math_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("dmr_site_math_host")
    base = ["g++", "-O0", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "modkit_amd", "csrc"),
            "-I", os.path.join(ROOT, "include")]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        san = []   # no sanitizer runtime on this machine: the same checks without it
    exe = d / "dmr_site_math_host"
    subprocess.check_call(base + san + ["-o", str(exe), os.path.join(ROOT, "tests", "dmr_site_math_host.cpp")])

    def run(lines):
        scn = d / "cases.txt"
        scn.write_text("\n".join(lines) + "\n")
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("MKP_")}
        p = subprocess.run([str(exe), str(scn)], capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        return p.stdout.splitlines()
    return run


def test_standalone_program_agrees_with_the_library(math_program):
    """the headers alone, sanitized: seeded counts up to 2^32 give the library's values bit for bit, and the planner the library's entries"""
    rng = random.Random(5)
    lines, want = ["g"], []
    for _ in range(300):
        big = rng.choice([10, 300, 5000, 2 ** 32 - 1])
        tot = [rng.randint(0, big) for _s in range(2)]
        cnt = [[0, 0], [0, 0]]
        has = [rng.randint(1, 3), rng.randint(1, 3)]
        for s in range(2):
            left = tot[s] + (1 if rng.random() < 0.03 else 0)   # (now and then beyond the total: a failure)
            for k in range(2):
                if (has[s] >> k) & 1:
                    cnt[s][k] = rng.randint(0, left)
                    left -= cnt[s][k]
        mc = (rng.randint(1, 400), rng.randint(1, 400))
        lines.append("s 2 0.55 0.55 0.05 %d %d %d %d %d %d %d %d %d %d" % (mc[0], mc[1], has[0], tot[0], has[1], tot[1], cnt[0][0], cnt[1][0],
                                                                       cnt[0][1], cnt[1][1]))
        want.append(modkit_amd.host_dmr_site_score(cnt[0], has[0], tot[0], cnt[1], has[1], tot[1], max_coverages=mc))
    plans = [([25, 8, 31], [[4, 3, 2], [5], [0, 10, 1, 0]], 10), ([2 ** 32 - 1], [[2 ** 32 - 1]], 2 ** 32 - 1), ([7], [[0]], 100)]
    for lengths, counts, interval in plans:
        lines.append("p %d %d " % (interval, len(lengths)) + " ".join("%d %s" % (n, " ".join(map(str, c))) for n, c in zip(lengths, counts)))
    out = math_program(lines)
    g = [float.fromhex(v) for v in out[0].split()[1:]]
    x, w = modkit_amd.host_dmr_sites_gauss_legendre()
    assert g == x + w
    for line, (vals, failed) in zip(out[1:301], want):
        f = line.split()
        assert f[0] == "s" and int(f[1]) == int(failed)
        for got, key in zip(f[2:], ("score", "ln_effect", "ln_null", "map_pvalue", "effect_size")):
            assert same_float(float.fromhex(got) if got not in ("nan", "-nan") else math.nan, vals[key]), (line, vals)
    at = 301
    for lengths, counts, interval in plans:
        entries, nb = modkit_amd.host_dmr_sites_batches(lengths, counts, interval)
        head = out[at].split()
        assert head[0] == "p" and int(head[1]) == nb and int(head[2]) == len(entries)
        assert [tuple(map(int, l.split()[1:])) for l in out[at + 1:at + 1 + len(entries)]] == entries
        at += 1 + len(entries)
