"""Host halves of `dmr pair` (the regions BED, the score, the table: modkit_amd/csrc/mkp_dmr.hpp behind mkp_host_parse_dmr_regions,
mkp_host_dmr_judge and mkp_host_dmr_table) against the independent model of tests/dmr_pair_model.py, and that model against the
reference's own golden table.  tests/dmr_score_host.cpp runs the header alone under the address and undefined-behaviour sanitizers.
No device is needed."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

import dmr_pair_model as model
import modkit_amd
from dmr_pair_cases import GOLDEN, REGIONS, check_table, code_repr, golden_inputs, score_tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_results():
    a, b, regions, fasta = golden_inputs()
    return regions, model.regions_results(a, b, regions, fasta)


def test_model_reproduces_the_golden_columns(golden_results):
    regions, results = golden_results
    want_fields, _ = model.split_table(open(GOLDEN).read())
    got_fields, _ = model.split_table(model.table_text(regions, results))
    assert len(want_fields) == 6 and got_fields == want_fields


def test_model_reproduces_the_golden_scores(golden_results):
    regions, results = golden_results
    worst = check_table(open(GOLDEN).read(), regions, results)
    print("largest |model - golden| in units of 2^-52 * sum|lgamma|: %.3f" % worst)


def counts_dict(results, codes):
    """The dict RegionSet.write_dmr_table takes (without score and state), of model results; a region the model does not write for another
    reason than its counts keeps that reason through the flags"""
    n, k = len(results), len(codes)
    d = {"codes": [code_repr(c) for c in codes], "has_reference": np.ones(n, dtype=np.uint8)}
    for f, shape, dt in (("n_mod", (n, k), np.uint64), ("has_code", (n, k), np.uint8), ("total", (n,), np.uint64), ("n_rows", (n,), np.uint64),
                         ("bad", (n,), np.uint8), ("contig_has_rows", (n,), np.uint8)):
        d[f] = [np.zeros(shape, dtype=dt) for _ in range(2)]
    for r, res in enumerate(results):
        for s, key in enumerate(("a", "b")):
            d["contig_has_rows"][s][r] = res["state"] != model.NO_CONTIG
            d["bad"][s][r] = res["state"] == model.BAD
            if key in res:
                counts, total, rows = res[key]
                d["total"][s][r], d["n_rows"][s][r] = total, rows
                for c, v in counts.items():
                    d["n_mod"][s][r, codes.index(c)], d["has_code"][s][r, codes.index(c)] = v, 1
        d["has_reference"][r] = res["state"] != model.NO_REFERENCE
    return d


def test_host_table_writer_gives_the_models_text(golden_results, tmp_path):
    regions, results = golden_results
    rs = modkit_amd.RegionSet(REGIONS, ["chr20"], dmr=True)
    for header in (False, True):
        out = tmp_path / "t.bed"
        rs.write_dmr_table(counts_dict(results, ["C"]), out, header=header)
        text = out.read_text()
        check_table(text, regions, results, header)
        if header:
            assert text.startswith(model.HEADER)
    fields, _ = model.split_table(text, True)
    assert fields == model.split_table(open(GOLDEN).read())[0]


# ---- the stand-alone program
@pytest.fixture(scope="module")
def score_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("dmr_score_host")
    base = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "modkit_amd", "csrc"), "-I",
            os.path.join(ROOT, "include")]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        san = []   # no sanitizer runtime on this machine: the same checks without it
    exe = d / "dmr_score_host"
    subprocess.check_call(base + san + ["-o", str(exe), os.path.join(ROOT, "tests", "dmr_score_host.cpp")])
    count = [0]

    def run(codes, cases, floats=()):
        """cases: [(a counts {code: n}, a total, b counts, b total, flags {a_bad, b_bad, a_contig, b_contig, has_ref, rule, named})]"""
        count[0] += 1
        codes = sorted(codes, key=model.code_key)   # the columns come in ModCodeRepr order
        words = [len(cases), len(codes)] + [code_repr(c) for c in codes]
        for i, (ac, at, bc, bt, fl) in enumerate(cases):
            words += [10 * i, 10 * i + 7, fl.get("rule", 3), fl.get("named", 1), at, bt, fl.get("a_bad", 0), fl.get("b_bad", 0), fl.get("a_contig", 1),
                      fl.get("b_contig", 1), fl.get("has_ref", 1)]
            for c in codes:
                words += [int(c in ac), ac.get(c, 0), int(c in bc), bc.get(c, 0)]
        scn = d / ("cases%d.txt" % count[0])
        scn.write_text(" ".join(str(w) for w in words) + "\n" + "".join("f %s\n" % f for f in floats))
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("MKP_")}
        p = subprocess.run([str(exe), str(scn)], capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = p.stdout.split("\n")
        at = lines.index("TABLE")
        states = [(int(l.split()[1]), float(l.split()[2]), l.split()[3]) for l in lines[:at]]
        rest = lines[at + 1:]
        table = [l for l in rest if l and not l.startswith("F ")]
        return states, "".join(l + "\n" for l in table), [l[2:] for l in rest if l.startswith("F ")]
    return run


def model_of_cases(cases):
    regions, results = [], []
    for i, (ac, at, bc, bt, fl) in enumerate(cases):
        start, end = 10 * i, 10 * i + 7
        regions.append(("c0", start, end, "r%d x" % i if fl.get("named", 1) else "c0:%d-%d" % (start, end), "?+-."[fl.get("rule", 3)]))
        if not (fl.get("a_contig", 1) and fl.get("b_contig", 1)):
            results.append({"state": model.NO_CONTIG})
        elif not fl.get("has_ref", 1):
            results.append({"state": model.NO_REFERENCE})
        elif fl.get("a_bad", 0) or fl.get("b_bad", 0):
            results.append({"state": model.BAD})
        else:
            ratio = model.llk_ratio(ac, at, bc, bt)
            results.append({"state": model.MODEL} if ratio is None else {"state": model.WRITTEN, "a": (ac, at, 0), "b": (bc, bt, 0), "score": ratio[0],
                                                                           "terms": ratio[1]})
    return regions, results


def check_cases(score_program, codes, cases):
    states, table, _ = score_program(codes, cases)
    regions, results = model_of_cases(cases)
    assert [s[0] for s in states] == [r["state"] for r in results]
    for (state, value, text), res in zip(states, results):
        if state == model.WRITTEN:
            assert abs(value - res["score"]) <= score_tolerance(res["terms"])
            assert float(text) == value and "e" not in text.lower()   # the printed score parses back to the same f64
    check_table(table, regions, results, header=True)
    return states, table


def test_score_branches(score_program):
    cases = [
        ({}, 0, {}, 0, {}),                                        # both samples empty: n_categories 1, score 0, `.` and NaN
        ({}, 0, {"m": 3}, 10, {}),                                 # one side empty: Beta branch over the other side's code
        ({"m": 4}, 9, {"h": 2}, 7, {}),                            # one code against a different code: the reference fails, region dropped
        ({"m": 4}, 9, {"m": 2}, 7, {}),                            # Beta
        ({"h": 0, "m": 4}, 9, {"m": 2}, 7, {}),                    # a zero-count code in the key set switches Beta to Dirichlet, k = 3
        ({"h": 1, "m": 4}, 9, {"h": 3, "m": 2}, 7, {}),            # k = 3
        ({"h": 1, "m": 4}, 9, {"a": 3, "m": 2}, 7, {}),            # k = 4: the union, not the larger key set, sizes the Dirichlet
        ({"21839": 2, "m": 1}, 5, {"m": 2}, 6, {}),                # a ChEBI code sorts behind the letters
        ({"m": 4}, 9, {"m": 2}, 7, {"a_bad": 1}), ({"m": 4}, 9, {"m": 2}, 7, {"b_contig": 0}), ({"m": 4}, 9, {"m": 2}, 7, {"has_ref": 0}),
        ({"m": 4}, 9, {"m": 2}, 7, {"named": 0, "rule": 1}), ({"m": 4}, 9, {"m": 2}, 7, {"rule": 2}),
        ({"m": 12}, 9, {"m": 2}, 7, {}),                           # more modified than total: AggregatedCounts::try_new fails
    ]
    states, table = check_cases(score_program, ["h", "m", "a", "21839"], cases)
    assert [s[0] for s in states] == [0, 0, 4, 0, 0, 0, 0, 0, 3, 1, 2, 0, 0, 4]
    assert states[0][2] == "0" and "\t.\t0\t.\t0\t.\t.\tNaN\tNaN\n" in table
    assert states[4][1] != states[3][1]                            # the zero-count code changed the model
    assert "21839:2" in table and table.index("m:1") < table.index("21839:2")
    assert "\tc0:110-117\t" in table and "\t+\t" in table and "\t-\t" in table


def test_seeded_counts_and_large_totals(score_program):
    rng = random.Random(20260)
    codes = ["h", "m", "a"]
    cases = []
    for i in range(300):
        def side():
            keys = rng.sample(codes, rng.randint(0, 3))
            top = rng.choice([0, 1, 5, 1000, (1 << 32) - 3, (1 << 32) + 5, 3 * (1 << 32)])
            counts = {c: rng.randint(0, max(top, 1)) // max(len(keys), 1) for c in keys}
            return counts, sum(counts.values()) + (rng.randint(0, max(top, 1)) if rng.random() < 0.8 else 0)
        (ac, at), (bc, bt) = side(), side()
        cases.append((ac, at, bc, bt, {"named": i % 2}))
    states, _ = check_cases(score_program, codes, cases)
    assert sum(1 for s in states if s[0] == 0) > 150


def test_f64_text(score_program):
    values = ["0", "-0.0", "-1.5", "1e-8", "0x1p-30", "123456789012345678", "1e17", "1.7976931348623157e308", "5e-324", "nan", "257.34514203447543",
              "-0.13968153023233754", "0.1"]
    _, _, texts = score_program(["m"], [({}, 0, {}, 0, {})], values)
    assert len(texts) == len(values)
    for raw, text in zip(values, texts):
        v = float.fromhex(raw) if raw.startswith("0x") else float(raw)
        assert text == model.f64_display(v), (raw, text)
        if v == v:
            assert "e" not in text.lower() and float(text) == v and math.copysign(1, float(text)) == math.copysign(1, v)
    assert texts[0] == "0" and texts[1] == "-0" and texts[3] == "0.00000001" and texts[6] == "100000000000000000" and texts[9] == "NaN"


# ---- the regions file
def test_regions_file_with_blank_holding_names(tmp_path):
    rs = modkit_amd.RegionSet(REGIONS, ["chr20"], dmr=True)
    want = model.parse_regions(open(REGIONS).read())
    assert len(want) == 6 and want[0][3] == "CpG: 47"
    assert [(c, s, e, n if n != "." else "%s:%d-%d" % (c, s, e), st) for c, s, e, n, st in rs.regions] == want
    p = tmp_path / "r.bed"
    text = "#chrom\tstart\tend\n# second\nchr1\t5\t9\tan island\t0\t-\nchrX 7 8\tq\t.\t+\nchr1\t1\t2\n"
    p.write_text(text)
    with pytest.raises(modkit_amd.MkpError):   # the stranded parser was picked: the last line has no strand
        modkit_amd.RegionSet(p, ["chr1"], dmr=True)
    p.write_text(text[:-len("chr1\t1\t2\n")])
    rs = modkit_amd.RegionSet(p, ["chr1"], dmr=True)
    assert rs.regions == [("chr1", 5, 9, "an island", "-"), ("chrX", 7, 8, "q", "+")] and rs.tids == [0, -1]
    assert [r[:3] + r[4:] for r in model.parse_regions(p.read_text())] == [r[:3] + r[4:] for r in rs.regions]
    for bad in ("", "#only\n", "chr1\t1\t2\n#late\n", "chr1\t9\t3\n"):
        p.write_text(bad)
        with pytest.raises(modkit_amd.MkpError):
            modkit_amd.RegionSet(p, ["chr1"], dmr=True)
        if bad != "chr1\t9\t3\n":
            with pytest.raises(model.RegionsError):
                model.parse_regions(bad)


# ---- refusals that need no device
def test_argument_refusals(tmp_path):
    base = ["-a", "a.bed", "-b", "b.bed", "-r", "r.bed", "--ref", "ref.fa", "--base", "C"]
    def refused(argv, status, word):
        with pytest.raises(modkit_amd.MkpError) as e:
            modkit_amd.dmr_pair(argv)
        assert e.value.status == status and word in str(e.value), str(e.value)
    refused(["-a", "a.bed", "-b", "b.bed", "--ref", "ref.fa", "--base", "C"], -3, "-r")
    refused(base + ["--segment", "seg.bed"], -3, "--segment")
    refused(base + ["-a", "a2.bed"], -3, "use modkit dmr multi")
    refused(base + ["-b", "b2.bed"], -3, "use modkit dmr multi")
    refused(base[:-2], -1, "at least 1 modified base")
    refused(base[:-1] + ["N"], -1, "A, C, G, or T")
    refused(base + ["--assign-code", "x"], -1, "invalid assignment")
    refused(base + ["--assign-code", "x:CC"], -1, "invalid assignment")
    refused(base + ["--missing", "loud"], -1, "--missing")
    refused(base + ["--cap-coverages"], -1, "unexpected argument")
    out = tmp_path / "exists.bed"
    out.write_text("keep\n")
    refused(base + ["-o", str(out)], -2, "refusing to overwrite")
    assert out.read_text() == "keep\n"
    exe = os.path.join(ROOT, "modkit_amd", "csrc", "mkpileup")
    p = subprocess.run([exe, "dmr", "multi", "-s", "a.bed", "x"], capture_output=True, text=True)
    assert p.returncode == 1 and "dmr multi" in p.stderr and "status -3" in p.stderr
