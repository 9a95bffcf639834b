"""Host halves of `dmr replicates` (modkit_amd/csrc/mkp_dmr_reps_math.hpp and mkp_dmr_reps.hpp behind mkp_host_dmr_reps_balance,
mkp_host_dmr_reps_pct, mkp_host_dmr_reps_table and the argument parser of mkp_dmr_reps_main) against the independent model of
tests/dmr_reps_model.py, and that model pinned: against dmr_sites_model on the lung tables, on sites worked by hand, and on the seeded sets
the device tests use (they tell f32 from f64 arithmetic, and they stay inside the caps on left-out sites).  tests/dmr_reps_math_host.cpp
runs the arithmetic header alone under the address and undefined-behaviour sanitizers.  No device is needed."""
import math
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import dmr_reps_model as model
import dmr_sites_model as sites_model
import modkit_amd
from dmr_pair_cases import code_repr, golden_inputs
from dmr_reps_cases import CAP_EVALUATIONS, CAP_SITES, SEEDS, fuzz_tables, left_out_of, site

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDED_KW = dict(n_sample=300, interval=50, batch_size=2)


# ---- the model, pinned
def test_model_equals_the_sites_model_on_the_lung_tables():
    a, b, _regions, fasta = golden_inputs()
    one, two = sites_model.run(a, b, fasta), model.run([a], [b], fasta)
    assert len(one["sites"]) > 10000 and len(two["sites"]) == len(one["sites"])
    for k in ("max_coverages", "n_sampled", "n_batches", "n_batches_dropped", "n_model_failures"):
        assert one[k] == two[k]
    for s, t in zip(one["sites"], two["sites"]):
        for k in ("chrom", "pos", "strand", "a", "b", "score", "terms", "pmap"):
            assert s[k] == t[k] or (k == "pmap" and repr(s[k]) == repr(t[k]))
        assert repr(t["balanced"]) == repr(t["pmap"]) and t["pct"] == (100, 100) and t["reps"] is None
    assert model.table_text(two) == sites_model.table_text(one["sites"]) and model.header(1, 1) == sites_model.HEADER


def test_sites_worked_by_hand():
    # a = {m 7 of 10, m 3 of 25}: target 35 / 2 = 17.5; 0.7 * 17.5 = 12.25 -> 12, 0.12 * 17.5 = 2.1 -> 2; totals 17 + 17
    assert model.collapse([({"m": 7}, 10), ({"m": 3}, 25)], True) == ({"m": 14}, 34, True)
    assert model.collapse([({"m": 7}, 10), ({"m": 3}, 25)], False) == ({"m": 10}, 35, True)
    # one present sample is cloned, whatever the other side holds
    assert model.collapse([({"h": 1, "m": 4}, 9)], True) == ({"h": 1, "m": 4}, 9, True)
    # a sample with total 0: 0 / 0 is NaN and casts to 0; target 10 / 2 = 5: 0 of 5 and floor(0.5 * 5) = 2 of 5
    assert model.collapse([({"m": 0}, 0), ({"m": 5}, 10)], True) == ({"m": 2}, 10, True)
    # three samples, two codes, key sets that differ: target 60 / 3 = 20; (3, 6) of 12 -> 5, 10; h 0 of 18 -> 0; m 30 of 30 -> 20
    assert model.collapse([({"h": 3, "m": 6}, 12), ({"h": 0}, 18), ({"m": 30}, 30)], True) == ({"h": 5, "m": 30}, 60, True)
    # a target that is no whole number: 31 / 3 = 10.333333 -> each total 10; 10 of 10 -> floor(10.333333) = 10
    assert model.collapse([({"m": 10}, 10), ({"m": 0}, 10), ({"m": 11}, 11)], True) == ({"m": 20}, 30, True)
    assert [model.pct_samples(k, 3) for k in (1, 2, 3)] == [33, 66, 100] and model.pct_samples(1, 16) == 6 and model.pct_samples(7, 7) == 100
    # 1 against 3: the clone rule on a, balance on b; unmatched, so no replicate values
    s = model.score_site([({"m": 4}, 9)], [({"m": 7}, 10), ({"m": 3}, 25), ({"m": 0}, 4)], 1, 3, (0.55, 0.55), 0.05, (300, 300))
    assert s["bal_a"] == ({"m": 4}, 9) and s["a"] == ({"m": 4}, 9) and s["reps"] is None and s["pct"] == (100, 100)
    # target 39 / 3 = 13: 0.7 * 13 = 9.1 -> 9; 0.12 * 13 = 1.56 -> 1; 0 -> 0; totals 13 each
    assert s["bal_b"] == ({"m": 10}, 39) and s["b"] == ({"m": 10}, 39)
    assert s["pmap"]["effect"] == 4 / 9 - 10 / 39 == s["balanced"]["effect"]
    # matched 2 against 2 with one b sample missing: no replicate values; with both: pairing by rank
    two = [({"m": 7}, 10), ({"m": 3}, 25)]
    assert model.score_site(two, two[:1], 2, 2, (0.55, 0.55), 0.05, (300, 300))["reps"] is None
    s = model.score_site(two, two[::-1], 2, 2, (0.55, 0.55), 0.05, (300, 300))
    assert [r["effect"] for r in s["reps"]] == [7 / 10 - 3 / 25, 3 / 25 - 7 / 10] and s["pmap"]["effect"] == 0.0 and s["pct"] == (100, 100)
    # a failing replicate pair fails the site, though the collapsed counts are fine
    bad = [({"m": 11}, 10), ({"m": 0}, 25)]
    assert model.collapse(bad, False) == ({"m": 11}, 35, True) and model.score_site(bad, two, 2, 2, (0.55, 0.55), 0.05, (300, 300)) is None
    assert model.score_site(bad, two, 2, 3, (0.55, 0.55), 0.05, (300, 300)) is None   # (unmatched: the balanced counts fail instead: 1.1 * 17.5 > 17)


@pytest.fixture(scope="module")
def seeded_results():
    return [(seed, fuzz_tables(seed)) for seed in SEEDS]


def test_seeded_sets_stay_inside_the_caps_and_tell_f32_from_f64(seeded_results):
    """before any device run, with the model alone: every seeded set leaves out at most 1 % of its evaluations and 3 % of its sites; and the
    sets hold sites whose balanced counts would differ had the reference worked in f64 (otherwise the f32 rule would go untested)"""
    differ = every = subsets = 0
    shapes = set()
    for seed, (a, b, fasta) in seeded_results:
        res = model.run(a, b, fasta, **SEEDED_KW)
        out = left_out_of(res)
        assert out[1] > 150 and out[0] <= CAP_SITES * out[1] and out[2] <= CAP_EVALUATIONS * out[3], (seed, out)
        shapes.add((len(a), len(b)))
        for s in res["sites"]:
            every += sum(1 for side in range(2) if len(s["present"][side]) > 1)
            subsets += len(s["present"][0]) != len(s["present"][1])
        differ += f64_differences(a, b, res)
    print("seeded sets: %d balanced sides of several samples, %d differ in f64; shapes %s" % (every, differ, sorted(shapes)))
    assert differ > 20 and subsets > 1000
    assert any(x == y for x, y in shapes) and any(x != y for x, y in shapes)


def f64_differences(a, b, res):
    """the balanced sides of the written sites whose counts an f64 evaluation would floor differently (from the samples' own rows again)"""
    n, index = 0, [{}, {}]
    for side, tables in enumerate((a, b)):
        for t, recs in enumerate(tables):
            for chrom, pos, code, _st, nv, nm, _nc in recs:
                index[side].setdefault((chrom, pos), {}).setdefault(t, ({}, nv))[0][code] = nm
    for s in res["sites"]:
        for side, key in ((0, "bal_a"), (1, "bal_b")):
            held = index[side].get((s["chrom"], s["pos"]), {})
            samples = [held[t] for t in s["present"][side]]
            if len(samples) > 1:
                assert model.collapse(samples, True)[:2] == s[key]
                n += model.collapse_f64(samples) != s[key]
    return n


# ---- the library's host functions against the model
def test_host_balance_against_the_model():
    rng = random.Random(17)
    codes = ["h", "m", "21839"]
    n_fail = n_nan = 0
    for case in range(4000):
        n = rng.randint(1, 7)
        big = rng.choice([20, 60, 60, 300, 5000, 2 ** 32 - 1])
        samples = []
        for _s in range(n):
            tot = rng.randint(0, big)
            keys = sorted(rng.sample(codes, rng.randint(1, 3)), key=code_repr)
            left, c = tot, {}
            for k in keys:
                c[k] = rng.randint(0, left)
                left -= c[k]
            samples.append((c, tot))
        cols = sorted(codes, key=code_repr)
        want_c, want_t, want_ok = model.collapse(samples, True)
        got_c, got_has, got_t, failed = modkit_amd.host_dmr_reps_balance(
            [[c.get(k, 0) for k in cols] for c, _t in samples], [sum(1 << j for j, k in enumerate(cols) if k in c) for c, _t in samples],
            [t for _c, t in samples])
        assert failed == (not want_ok)
        assert got_t == want_t and got_has == sum(1 << j for j, k in enumerate(cols) if k in want_c)
        assert got_c == [want_c.get(k, 0) for k in cols], (samples, got_c, want_c)
        n_fail += failed
        n_nan += any(t == 0 for _c, t in samples) and n > 1
    assert n_nan > 20
    # beyond its total a sample's balanced counts exceed the balanced total: where the reference aborts
    assert modkit_amd.host_dmr_reps_balance([[11], [0]], [1, 1], [10, 25])[3] and not model.collapse([({"m": 11}, 10), ({"m": 0}, 25)], True)[2]
    assert modkit_amd.host_dmr_reps_balance([[7], [3]], [1, 1], [10, 25]) == ([14], 1, 34, False)
    for n in range(1, 17):
        for k in range(0, n + 1):
            assert modkit_amd.host_dmr_reps_pct(k, n) == model.pct_samples(k, n)


def table_dict(res, names, codes):
    sites = res["sites"]
    n_a = res["n_a"]
    d = {"codes": [code_repr(c) for c in codes], "tid": [names.index(s["chrom"]) for s in sites], "pos": [s["pos"] for s in sites],
         "strand": "".join(s["strand"] for s in sites), "score": [s["score"] for s in sites], "map_pvalue": [s["pmap"]["p"] for s in sites],
         "effect_size": [s["pmap"]["effect"] for s in sites], "n_a": n_a, "n_b": res["n_b"],
         "balanced_map_pvalue": [s["balanced"]["p"] for s in sites], "balanced_effect_size": [s["balanced"]["effect"] for s in sites],
         "pct_samples": ([s["pct"][0] for s in sites], [s["pct"][1] for s in sites]), "n_rep": [len(s["reps"] or []) for s in sites],
         "total": [], "n_mod": [], "has_code": []}
    for key in ("a", "b"):
        d["total"].append([s[key][1] for s in sites])
        d["n_mod"].append([[s[key][0].get(c, 0) for c in codes] for s in sites])
        d["has_code"].append([sum(1 << k for k, c in enumerate(codes) if c in s[key][0]) for s in sites])
    for f, key in (("rep_pvalue", "p"), ("rep_effect", "effect")):
        d[f] = [[(s["reps"][r][key] if s["reps"] and r < len(s["reps"]) else 0.0) for r in range(n_a)] for s in sites]
    return d


def test_table_writer_for_the_three_header_shapes(tmp_path):
    pm = lambda p, e: {"p": p, "effect": e, "ln_effect": None, "ln_null": None, "s_effect": 0.0, "s_null": 0.0, "top": None}
    def mk(pos, reps, pct=(100, 50), chrom="chrB", strand="+", p=0.25, e=-0.125, bal=(math.nan, math.nan)):
        return {"chrom": chrom, "pos": pos, "strand": strand, "a": ({"h": 1, "m": 2}, 7), "b": ({"m": 0}, 0), "score": 1.5, "terms": 0.0,
                "pmap": pm(p, e), "balanced": pm(*bal), "pct": pct, "reps": reps}
    names, codes = ["chrA", "chrB"], ["h", "m"]
    shapes = {(1, 1): [], (2, 3): ["balanced_map_pvalue", "balanced_effect_size", "pct_a_samples", "pct_b_samples"]}
    shapes[(3, 3)] = shapes[(2, 3)] + ["replicate_map_pvalues", "replicate_effect_sizes"]
    for (n_a, n_b), extra in shapes.items():
        sites = [mk(5, None), mk(9, [pm(1.0, 0.05)], pct=(33, 33), strand="-", bal=(0.0, 1.0)),
                 mk(11, [pm(6.230948043897502e-07, 1.0 / 3.0), pm(math.nan, math.nan), pm(1e-7, -1.0)], pct=(100, 100), chrom="chrA")]
        if n_a != n_b:
            for s in sites:
                s["reps"] = None
        res = {"sites": sites, "n_a": n_a, "n_b": n_b}
        for with_header in (False, True):
            out = tmp_path / "t.bed"
            modkit_amd.write_dmr_reps_table(table_dict(res, names, codes), names, out, header=with_header)
            assert out.read_text() == model.table_text(res, with_header)
        lines = out.read_text().splitlines()
        assert lines[0].split("\t")[16:] == extra and all(len(l.split("\t")) == 16 + len(extra) for l in lines)
        if (n_a, n_b) == (1, 1):
            assert out.read_text() == sites_model.table_text(sites, True)
        if (n_a, n_b) == (2, 3):
            assert lines[1].endswith("\t0.25\t-0.125\tNaN\tNaN\t100\t50") and lines[2].endswith("\t0\t1\t33\t33")
        if (n_a, n_b) == (3, 3):
            assert lines[1].endswith("\t100\t50\t-\t-") and lines[2].endswith("\t33\t33\t1\t0.05")   # (a one-element list)
            assert lines[3].endswith("\t0.0000006230948043897502,NaN,0.0000001\t0.3333333333333333,NaN,-1")


def test_argument_refusals(tmp_path):
    base = ["-a", "a.bed", "-b", "b.bed", "--ref", "ref.fa", "--base", "C"]
    def refused(argv, status, word):
        with pytest.raises(modkit_amd.MkpError) as e:
            modkit_amd.dmr_replicates(argv)
        assert e.value.status == status and word in str(e.value), str(e.value)
    refused(base + ["-a", "a2.bed", "-r", "r.bed"], -1, "dmr pair")
    refused(base + ["-b", "b2.bed", "--segment", "seg.bed"], -3, "--segment")
    refused([x for k in range(17) for x in ("-a", "a%d.bed" % k)] + base[2:], -3, "at most 16")
    refused([x for k in range(17) for x in ("-b", "b%d.bed" % k)] + base[:2] + base[4:], -3, "at most 16")
    refused(base[2:], -1, "at least 1 'a' sample")
    refused(base[:2] + base[4:], -1, "at least 1 'a' sample")
    refused(base + ["--frobnicate"], -1, "for dmr replicates")
    refused(base + ["--max-coverages", "30", "30", "-N", "100"], -1, "cannot be used with")
    out = tmp_path / "exists.bed"
    out.write_text("keep\n")
    refused(base + ["-a", "a2.bed", "-o", str(out)], -2, "refusing to overwrite")   # (a second -a is accepted)
    assert out.read_text() == "keep\n"
    # dmr sites still refuses a second table, and names the command that takes it
    with pytest.raises(modkit_amd.MkpError) as e:
        modkit_amd.dmr_sites(base + ["-a", "a2.bed"])
    assert e.value.status == -3 and "replicates" in str(e.value) and "dmr replicates" in str(e.value)
    exe = os.path.join(ROOT, "modkit_amd", "csrc", "mkpileup")
    p = subprocess.run([exe, "dmr", "replicates"] + base + ["-r", "r.bed"], capture_output=True, text=True)
    assert p.returncode == 1 and "dmr pair" in p.stderr and "status -1" in p.stderr


# ---- the stand-alone program
def test_standalone_program_agrees_with_the_library_and_the_model(tmp_path):
    """the arithmetic header alone, sanitized: seeded counts up to 2^32 give the library's and the model's balanced counts"""
    base = ["g++", "-O0", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "modkit_amd", "csrc"),
            "-I", os.path.join(ROOT, "include")]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        san = []   # no sanitizer runtime on this machine: the same checks without it
    exe = tmp_path / "dmr_reps_math_host"
    subprocess.check_call(base + san + ["-o", str(exe), os.path.join(ROOT, "tests", "dmr_reps_math_host.cpp")])
    rng = random.Random(23)
    lines, want = [], []
    for _ in range(600):
        n, nc = rng.randint(1, 16), rng.randint(1, 3)
        big = rng.choice([10, 60, 300, 5000, 2 ** 32 - 1])
        rows, samples = [], []
        for _s in range(n):
            tot = rng.randint(0, big)
            has = rng.randint(1, (1 << nc) - 1)
            left = tot + (1 if tot and rng.random() < 0.02 else 0)   # (now and then beyond the total)
            cnt = [0] * nc
            for k in range(nc):
                if (has >> k) & 1:
                    cnt[k] = rng.randint(0, left)
                    left -= cnt[k]
            rows.append("%d %d %s" % (has, tot, " ".join(map(str, cnt))))
            samples.append(({k: cnt[k] for k in range(nc) if (has >> k) & 1}, tot))
        lines.append("b %d %d %s" % (n, nc, " ".join(rows)))
        c, t, ok = model.collapse(samples, True)
        want.append("b %d %d %d %s" % (0 if ok else 1, sum(1 << k for k in c), t, " ".join(str(c.get(k, 0)) for k in range(nc))))
    for n in range(1, 17):
        for k in range(n + 1):
            lines.append("c %d %d" % (k, n))
            want.append("c %d" % model.pct_samples(k, n))
    for x, count in ((math.nan, 0), (math.inf, 2 ** 64 - 1), (-math.inf, 0), (-1.0, 0), (0.0, 0), (3.0, 3), (2.0 ** 64, 2 ** 64 - 1), (2.0 ** 63, 2 ** 63),
                     (4294967296.0, 2 ** 32)):
        lines.append("f %x" % struct.unpack("<I", struct.pack("<f", x))[0])
        want.append("f %d" % count)
    scn = tmp_path / "cases.txt"
    scn.write_text("\n".join(lines) + "\n")
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("MKP_")}
    p = subprocess.run([str(exe), str(scn)], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.splitlines() == want
