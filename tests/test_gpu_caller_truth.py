"""The device's threshold callers against the independent f32 model (tests/caller_model.py) on the truth-table modBAMs of
tests/caller_truth_cases.py — not against the oracle: every ML byte, every (h, m) pair, thresholds at and one f32 ulp beside call
probabilities, collapse shares over 1-4 entries, ties, per-base / per-mod lookups, every decode class.  Paths: the fused slot decoder
(integer caller and f32 walk), the event decoders (MKP_FUSED=0), the dense path without focus positions, `extract calls`, `summary`,
threshold estimation and `sample-probs`.  Calls whose answer depends on the map's iteration order are compared with the oracle."""
import os
import subprocess

import numpy as np
import pytest

import caller_model as model
import caller_truth_cases as tc
import modkit_amd

pytestmark = pytest.mark.gpu

_BAMS = {}


def _bam(tmp_path_factory, name):
    if name not in _BAMS:
        ml, solo = tc.ml_content(name)
        d = tmp_path_factory.mktemp("truth_" + name)
        bam, fa, calls = tc.TruthBam(name, ml, solo, seed=21).write(str(d / name))
        _BAMS[name] = (ml, solo, bam, fa, calls, d)
    return _BAMS[name]


def _pileup(bam, out, flags, fused=True):
    old = os.environ.get("MKP_FUSED")
    try:
        if fused:
            os.environ.pop("MKP_FUSED", None)
        else:
            os.environ["MKP_FUSED"] = "0"
        modkit_amd.pileup([bam, out] + flags)
    finally:
        if old is None:
            os.environ.pop("MKP_FUSED", None)
        else:
            os.environ["MKP_FUSED"] = old


PATHS = {
    "fused": (["--cpg", "--ref", "{fa}"], True),     # the fused slot decoder (classes 0 and 1), event decoders for the rest
    "events": (["--cpg", "--ref", "{fa}"], False),   # every class through the event decoders
    "dense": ([], True),                             # no focus positions: mkp_pileup_tiles
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(tc.LAYOUTS))
def test_pileup_calls_match_model(oracle_bin, tmp_path_factory, name, path):
    ml, solo, bam, fa, calls, d = _bam(tmp_path_factory, name)
    base_flags, fused = PATHS[path]
    n_dep = 0
    for si, spec in enumerate(tc.specs_for(name)):
        if path == "dense" and spec.traditional:
            continue   # (the preset implies --cpg)
        flags = [f.format(fa=fa) for f in base_flags] + spec.flags()
        if spec.traditional:
            flags += ["--ref", fa] if "--ref" not in flags else []
        exp = tc.expected_calls(name, ml, solo, calls, spec)
        out = str(d / ("%s_%d.bed" % (path, si)))
        _pileup(bam, out, flags, fused)
        got = tc.bed_calls(out, calls, combine=spec.traditional)
        want = tc.expected_bed(exp)
        dep = exp["order_dep"]
        if dep.any():   # order-dependent calls: the oracle's answer
            ora = str(d / ("%s_%d_oracle.bed" % (path, si)))
            p = subprocess.run([oracle_bin, "pileup", bam, ora] + flags, capture_output=True, text=True)
            assert p.returncode == 0, p.stderr[-300:]
            want = np.where(dep, tc.bed_calls(ora, calls, combine=spec.traditional), want)
            n_dep += int(dep.sum())
        msg = tc.first_mismatch("%s pileup" % path, got, want, np.zeros(len(got), bool), name, ml, solo, calls, spec)
        assert msg is None, msg
    print("layout %s, %s: %d order-dependent calls compared with the oracle" % (name, path, n_dep))


EXTRACT_SPECS = [tc.Spec(), tc.Spec(default=0.6, per_mod={"m": 0.7}), tc.Spec(default=float(model.quals_to_probs(128))),
                 tc.Spec(default=0.5, ignore="h"), tc.Spec(default=1.5)]


@pytest.mark.parametrize("name", ["m", "hm", "h_m", "m_dot", "h_m_dot", "hmfc", "chebi"])
def test_extract_calls_match_model(oracle_bin, tmp_path_factory, name):
    ml, solo, bam, fa, calls, d = _bam(tmp_path_factory, name)
    for si, spec in enumerate(EXTRACT_SPECS):
        out, ora = str(d / ("x%d.tsv" % si)), str(d / ("x%d_oracle.tsv" % si))
        modkit_amd.extract_calls([bam, out] + spec.flags())
        p = subprocess.run([oracle_bin, "extract-calls", bam, ora] + spec.flags(), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-300:]
        msg = tc.check_extract(out, name, ml, solo, calls, spec, oracle_path=ora)
        assert msg is None, msg


@pytest.mark.parametrize("ci", range(len(tc.SUMMARY_CASES)))
def test_summary_counts_match_model(tmp_path_factory, ci):
    name, spec = tc.SUMMARY_CASES[ci]
    ml, solo, bam, fa, calls, d = _bam(tmp_path_factory, name)
    exp = tc.expected_calls(name, ml, solo, calls, spec)
    assert not exp["order_dep"].any()
    ctx = modkit_amd.Context()
    try:
        got = ctx.summary(bam, ["--no-sampling"] + spec.flags())
    finally:
        ctx.close()
    assert tc.summary_rows(got) == tc.expected_summary(exp)


def _sample_bam(tmp_path, name, ml):
    bam, fa, calls = tc.TruthBam(name, ml, None, seed=22).write(str(tmp_path / ("s%d" % len(ml))))
    return bam, fa, calls


# samples: sizes whose (n - 1) q falls between order statistics in different level-0 histogram bins (the top 16 bits of the f32),
# between values of one bin (a collapse share), and samples of a single value
SAMPLES = [("m", np.arange(256, dtype=np.uint8).reshape(-1, 1)),
           ("m", np.array([[3], [250], [7]], np.uint8)),
           ("m", np.full((40, 1), 200, np.uint8)),
           ("m", np.full((2, 1), 0, np.uint8)),
           ("hm", tc.ml_content("hm")[0][::37]),
           ("hmf", tc.ml_content("hmf")[0][:999])]


@pytest.mark.parametrize("si", range(len(SAMPLES)))
def test_threshold_estimate_and_sample_probs_match_model(tmp_path, si):
    name, ml = SAMPLES[si]
    bam, fa, calls = _sample_bam(tmp_path, name, ml)
    solo = np.zeros((0, ml.shape[1]), np.uint8)
    exp = tc.expected_calls(name, ml, solo, calls, tc.Spec())
    xs = tc.argmax_sample(exp)
    qs = [0.1, 0.5, 0.33, 0.9, 0.0, 1.0]
    want = [model.percentile_linear_interp(xs, q) for q in qs]
    ctx = modkit_amd.Context()
    try:
        got = ctx.sample_probs(bam, qs, ["--no-sampling"])
        assert got["C"]["n"] == len(xs)
        assert [np.float32(v).view(np.uint32) for v in got["C"]["percentiles"].values()] == [np.float32(w).view(np.uint32) for w in want], \
            "sample-probs: got %s, model %s" % (list(got["C"]["percentiles"].values()), want)
        for q, w in zip((0.1, 0.5, 0.33), want):
            rep = ctx.pileup_run([bam, str(tmp_path / "est.bed"), "-f", "1.0", "-p", model.shortest(q)])
            t = rep.as_dict()["thresholds"]["C"]
            assert np.float32(t).view(np.uint32) == np.float32(w).view(np.uint32), "estimate at q=%s: got %r, model %r" % (q, t, w)
    finally:
        ctx.close()
