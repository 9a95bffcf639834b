"""The oracle's threshold caller against the independent f32 model (tests/caller_model.py) on the truth-table modBAMs of
tests/caller_truth_cases.py: every ML byte, every (h, m) pair, thresholds at and one ulp beside call probabilities, collapse shares
over 1-4 entries, ties, per-base / per-mod lookups.  This pins the oracle apart from its author's own reading of the reference."""
import subprocess

import numpy as np
import pytest

import caller_model as model
import caller_truth_cases as tc


def _oracle(oracle_bin, cmd, bam, out, flags):
    p = subprocess.run([oracle_bin, cmd, bam, out] + flags, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-400:]


@pytest.mark.parametrize("name", list(tc.LAYOUTS))
def test_oracle_pileup_matches_model(oracle_bin, tmp_path, name):
    ml, solo = tc.ml_content(name)
    bam, fa, calls = tc.TruthBam(name, ml, solo, seed=11).write(str(tmp_path / name))
    n_dep = 0
    for si, spec in enumerate(tc.specs_for(name)):
        exp = tc.expected_calls(name, ml, solo, calls, spec)
        out = str(tmp_path / ("o%d.bed" % si))
        _oracle(oracle_bin, "pileup", bam, out, ["--cpg", "--ref", fa] + spec.flags())
        got = tc.bed_calls(out, calls, combine=spec.traditional)
        msg = tc.first_mismatch("oracle pileup", got, tc.expected_bed(exp), exp["order_dep"], name, ml, solo, calls, spec)
        assert msg is None, msg
        n_dep += int(exp["order_dep"].sum())
    print("layout %s: %d order-dependent calls left to the oracle" % (name, n_dep))


@pytest.mark.parametrize("name", ["m", "hm", "h_m", "hmfc", "chebi"])
def test_oracle_extract_calls_matches_model(oracle_bin, tmp_path, name):
    ml, solo = tc.ml_content(name)
    bam, fa, calls = tc.TruthBam(name, ml, solo, seed=12).write(str(tmp_path / name))
    for si, spec in enumerate([tc.Spec(), tc.Spec(default=0.6, per_mod={"m": 0.7}), tc.Spec(default=0.5, ignore=tc.layout_codes(name)[0])]):
        out = str(tmp_path / ("o%d.tsv" % si))
        _oracle(oracle_bin, "extract-calls", bam, out, spec.flags())
        exp = tc.expected_calls(name, ml, solo, calls, spec)
        keep = dict(calls)
        msg = tc.check_extract(out, name, ml, solo, keep, spec) if not exp["order_dep"].any() else \
            tc.check_extract(out, name, ml, solo, keep, spec, oracle_path=out)
        assert msg is None, msg


def test_call_prob_text_is_the_shortest_repr():
    # extract calls' call_prob (Rust's `{}` of an f32): every (q + 0.5) / 256 and the values of a collapse share print as numpy's
    # shortest round-trip positional form, which reads back as the same f32
    vals = list(model.quals_to_probs(np.arange(256)))
    vals += [tc.share_value(a, b, n) for a in (0, 77, 255) for b in (0, 1, 200) for n in (1, 2, 3, 4)]
    for v in vals:
        s = model.shortest(v)
        assert np.float32(float(s)) == v and "e" not in s


@pytest.mark.parametrize("ci", range(len(tc.SUMMARY_CASES)))
def test_oracle_summary_matches_model(oracle_bin, tmp_path, ci):
    from test_oracle_golden import run_oracle_summary
    name, spec = tc.SUMMARY_CASES[ci]
    ml, solo = tc.ml_content(name)
    bam, fa, calls = tc.TruthBam(name, ml, solo, seed=13).write(str(tmp_path / name))
    exp = tc.expected_calls(name, ml, solo, calls, spec)
    assert not exp["order_dep"].any()
    got = run_oracle_summary(oracle_bin, bam, ["--no-sampling"] + spec.flags())
    assert tc.summary_rows(got) == tc.expected_summary(exp)


@pytest.mark.parametrize("q", [0.1, 0.5, 0.33, 0.9, 0.0])
def test_oracle_estimated_threshold_matches_model(oracle_bin, tmp_path, q):
    name = "hm"
    ml, solo = tc.ml_content(name)
    ml = ml[::37]   # 1772 pairs: (n - 1) q falls between two order statistics
    bam, fa, calls = tc.TruthBam(name, ml, solo, seed=14).write(str(tmp_path / name))
    exp = tc.expected_calls(name, ml, solo, calls, tc.Spec())
    want = model.percentile_linear_interp(tc.argmax_sample(exp), q)
    p = subprocess.run([oracle_bin, "sample-probs", bam, "-p", model.shortest(q), "--no-sampling"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-300:]
    b, _, v, n = p.stdout.splitlines()[0].split("\t")
    assert b == "C" and int(n) == len(calls["pos"]) and np.float32(float(v)) == want
