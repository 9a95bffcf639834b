"""An independent model of `modkit dmr pair -a A -b B --ref ref.fa --base C` WITHOUT -r (v0.4.4: src/dmr/single_site.rs, beta_diff.rs,
llr_model.rs, bedmethyl.rs, src/genome_positions.rs:91-127, src/thresholds.rs:17-38), written from those files and not from the library's
C++ or its kernels: bedMethyl records of two samples, the reference sequences and the options in; the written sites, the counters, the max
coverages and the table text out.  Everything is dicts and sorted lists; lgamma / log are math's, exp returns inf above 709.78 and lets NaN
through (as an IEEE exp does), the quadrature nodes are numpy's leggauss(16), f32 arithmetic is numpy.float32.

Per f64 value the model also returns its error unit S (the tests allow a multiple of 2^-52 * S): the sum of the absolute values of every
lgamma value, the two power terms, the ln of the integral and the largest exponent inside the quadrature."""
import math

import numpy as np

import dmr_pair_model as pair

DEFAULT_LOOKUP = pair.DEFAULT_LOOKUP
LOWER, UPPER = 1e-5, 1.0 - 1e-5
MAX_COV_ALLOWED = 300
GL_X, GL_W = (list(map(float, v)) for v in np.polynomial.legendre.leggauss(16))
EXP_OVERFLOW = 709.78
EXP_UNDERFLOW = -745.13


class ModelError(Exception):
    pass


def exp(x):
    if x != x:
        return x
    if x > EXP_OVERFLOW:
        return math.inf
    return math.exp(x)


def log(x):
    if x != x:
        return x
    if x == 0.0:
        return -math.inf
    if x == math.inf:
        return math.inf
    return math.log(x)


def lgamma(x):
    return x if x != x else math.lgamma(x)


def ln_beta(a, b):
    """(value, sum of |lgamma values|)"""
    t = [lgamma(a), lgamma(b), lgamma(a + b)]
    return t[0] + t[1] - t[2], sum(abs(v) for v in t)


def rust_round(x):
    """f64::round: half away from zero"""
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def resize(n_mod, cov, max_cov):
    frac = n_mod / cov if cov else math.nan
    if cov > max_cov:
        n = rust_round(frac * max_cov)
        return int(n), max_cov, n / max_cov
    return n_mod, cov, frac


def calc_beta_diff(d, p1, p2, delta):
    """(ln_p, S, largest exponent of the quadrature or None); None where the reference fails"""
    (a1, b1), (a2, b2) = p1, p2
    (la1, sa1), (la2, sa2) = ln_beta(a1, b1), ln_beta(a2, b2)
    ln_a, s_a = la1 + la2, sa1 + sa2
    if abs(d) < delta:
        if a1 + a2 < 1.0 or b1 + b2 < 1.0:
            return None
        v, s = ln_beta(a1 + a2 - 1.0, b1 + b2 - 1.0)
        return v - ln_a, s + s_a, None
    if d > 0.0:
        x, y, a, q1, q2, c = 1.0 - d, 1.0 - d * d, b1, a1 + b1 + a2 + b2 - 2.0, 1.0 - a1, a2 + b1
        (lb, s_lb), t1, t2 = ln_beta(a2, b1), log(d) * (b1 + b2 - 1.0), log(1.0 - d) * (a2 + b1 - 1.0)
    else:   # (a NaN lands here, as in the reference)
        x, y, a, q1, q2, c = 1.0 - d * d, 1.0 + d, b2, 1.0 - a2, a1 + b1 + a2 + b2 - 2.0, a1 + b2
        (lb, s_lb), t1, t2 = ln_beta(a1, b2), log(-d) * (b1 + b2 - 1.0), log(1.0 + d) * (a1 + b2 - 1.0)
    half_diff, half_sum = (UPPER - LOWER) / 2.0, (LOWER + UPPER) / 2.0
    total, top = 0.0, -math.inf
    for gx, gw in zip(GL_X, GL_W):
        u = half_diff * gx + half_sum
        ex = ((a - 1.0) * log(u) + (-a + c - 1.0) * log(1.0 - u)) - (q1 * log(1.0 - u * x) + q2 * log(1.0 - y * u))
        if ex == ex:
            top = max(top, ex)
        total += gw * exp(ex)
    ln_int = log(half_diff * total)
    corr, s_corr = ln_beta(a, c - a)
    ln_p = lb + t1 + t2 + (ln_int - corr) - ln_a
    s = s_lb + s_corr + s_a + abs(t1) + abs(t2) + (abs(ln_int) if math.isfinite(ln_int) else 0.0) + (abs(top) if math.isfinite(top) else 0.0)
    return ln_p, s, top


def pmap(a_mod, a_cov, b_mod, b_cov, prior=(0.55, 0.55), delta=0.05, max_cov=(300, 300)):
    """PMapEstimator::run: a dict with p, effect, ln_effect, ln_null (None where not computed), s_effect, s_null, top; None where it fails"""
    if a_mod > a_cov or b_mod > b_cov:
        return None
    a_mod, a_cov, fa = resize(a_mod, a_cov, min(max_cov[0], MAX_COV_ALLOWED))
    b_mod, b_cov, fb = resize(b_mod, b_cov, min(max_cov[1], MAX_COV_ALLOWED))
    e = fa - fb
    out = {"effect": e, "ln_effect": None, "ln_null": None, "s_effect": 0.0, "s_null": 0.0, "top": None}
    if abs(e) <= delta:
        out["p"] = 1.0
        return out
    d = e - 0.005 if e > 0.0 else e + 0.005
    p1, p2 = (prior[0] + a_mod, prior[1] + (a_cov - a_mod)), (prior[0] + b_mod, prior[1] + (b_cov - b_mod))
    eff = calc_beta_diff(d, p1, p2, delta)
    if eff is None:
        return None
    out["ln_effect"], out["s_effect"], out["top"] = eff
    if exp(eff[0]) == 0.0:
        out["p"] = 1.0
        return out
    null = calc_beta_diff(0.0, p1, p2, delta)
    if null is None:
        return None
    out["ln_null"], out["s_null"], _ = null
    p = exp(null[0] - eff[0])
    out["p"] = 1.0 if p > 1.0 else p
    return out


def flippable(r):
    """a pair whose branch could legitimately differ between two libms: left out of seeded comparisons"""
    if r is None or r["ln_effect"] is None:
        return False
    if r["top"] is not None and abs(r["top"] - EXP_OVERFLOW) < 1.0:
        return True
    if abs(r["ln_effect"] - EXP_UNDERFLOW) < 1.0:
        return True
    # (with |d| < delta both values are one expression evaluated twice: p is exactly 1 whatever the libm)
    if r["top"] is not None and r["ln_null"] is not None and math.isfinite(r["ln_effect"]) and \
            abs(r["ln_null"] - r["ln_effect"]) < 4.0 * 2.0 ** -52 * (r["s_effect"] + r["s_null"]):
        return True
    return False


# ---------------------------------------------------------------------------------------------- the walk
def listed_positions(seq, bases, mask):
    """get_positions(contig, whole contig, Both): {position: (strand, base)}; a base of the --base set is listed '+', otherwise a base of
    the complement set '-' (numpy over the bytes: a chromosome is too long for a Python loop)"""
    b = np.frombuffer(seq.encode(), dtype=np.uint8)
    if not mask:
        b = np.where((b >= ord("a")) & (b <= ord("z")), b - 32, b)
    plus = np.isin(b, [ord(x) for x in bases])
    minus = np.isin(b, [ord(pair.COMPLEMENT[x]) for x in bases]) & ~plus
    out = {int(p): ("+", chr(b[p])) for p in np.flatnonzero(plus)}
    out.update({int(p): ("-", chr(b[p])) for p in np.flatnonzero(minus)})
    return out


def walk_contigs(records_a, records_b, fasta):
    names = sorted(n for n in fasta if any(r[0] == n for r in records_a) and any(r[0] == n for r in records_b))
    return sorted(names, key=lambda n: n.encode())


def super_batches(contigs, listed, lengths, interval, batch_size):
    """SingleSiteBatches::get_next_batch, call by call: a list of super-batches, each a list of batches, each a list of (contig, start, end)"""
    queue = list(contigs)
    if not queue:
        raise ModelError("need at least 1 contig")
    cur, pos, done, out = queue.pop(0), 0, False, []
    while True:
        batches, current, length = [], [], 0
        while len(batches) < batch_size and not done:
            end = min(pos + interval, lengths[cur])
            current.append((cur, pos, end))
            arr = listed[cur + "#arr"]
            length += int(np.count_nonzero((arr >= pos) & (arr < end)))
            if length >= interval:
                batches.append(current)
                current, length = [], 0
            if end >= lengths[cur]:
                if queue:
                    cur, pos = queue.pop(0), 0
                else:
                    done = True
            else:
                pos = end
        if current:
            batches.append(current)
        if not batches:
            return out
        out.append(batches)


def percentile_linear_interp(xs, q):
    if len(xs) < 2:
        raise ModelError("too few data points to calculate percentile, got %d" % len(xs))
    l = np.float32(len(xs) - 1)
    lq = l * np.float32(q)
    left, right = int(np.floor(lq)), int(np.ceil(lq))
    g = lq - np.trunc(lq)
    return np.float32(xs[left]) * (np.float32(1) - g) + np.float32(xs[right]) * g


def run(records_a, records_b, fasta, bases=("C",), lookup=None, min_cov=0, mask=False, prior=(0.55, 0.55), delta=0.05, max_coverages=None,
        n_sample=10042, interval=100000, batch_size=6):
    """The whole run.  Returns {"sites": [site dict], "max_coverages", "n_sampled", "n_batches", "n_batches_dropped", "n_model_failures"}; a
    site = chrom, pos, strand, a / b = ({code: n_mod}, total), score, terms, pmap (the dict of pmap())."""
    lookup = DEFAULT_LOOKUP if lookup is None else lookup
    contigs = walk_contigs(records_a, records_b, fasta)
    if not contigs:
        raise ModelError("need at least 1 contig")
    listed, lengths = {}, {}
    for n in contigs:
        listed[n] = listed_positions(fasta[n], bases, mask)
        listed[n + "#arr"] = np.array(sorted(listed[n]), dtype=np.int64)
        lengths[n] = len(fasta[n])
    # the rows that take part, per sample and contig, ascending
    part = [{n: [] for n in contigs}, {n: [] for n in contigs}]
    for s, recs in enumerate((records_a, records_b)):
        for chrom, pos, code, strand, n_valid, n_mod, n_can in recs:
            if chrom not in part[s] or n_valid < min_cov or code not in lookup:
                continue
            st = "-" if strand == "-" else "+"
            base = pair.COMPLEMENT[lookup[code]] if st == "-" else lookup[code]
            if listed[chrom].get(pos) == (st, base):
                part[s][chrom].append((pos, st, code, n_valid, n_mod, n_can))
    supers = super_batches(contigs, listed, lengths, interval, batch_size)

    def rows_in(s, batch):
        return [r for chrom, lo, hi in batch for r in part[s][chrom] if lo <= r[0] < hi]

    n_sampled = (0, 0)
    if max_coverages is None:
        cov = [[], []]
        for sb in supers:
            for batch in sb:
                for s in range(2):
                    cov[s] += [r[3] for r in rows_in(s, batch)]
            if min(len(cov[0]), len(cov[1])) >= n_sample:
                break
        n_sampled = (len(cov[0]), len(cov[1]))
        max_coverages = tuple(int(np.floor(percentile_linear_interp(sorted(np.float32(v) for v in c), 0.95))) for c in cov)
    max_coverages = tuple(min(int(m), MAX_COV_ALLOWED) for m in max_coverages)

    sites, dropped, failures, n_batches = [], 0, 0, 0
    for sb in supers:
        for batch in sb:
            n_batches += 1
            agg, bad = [{}, {}], False
            for s in range(2):
                groups = {}
                for chrom, lo, hi in batch:
                    for r in part[s][chrom]:
                        if lo <= r[0] < hi:
                            groups.setdefault((chrom, r[0]), []).append(r)
                for key, g in groups.items():
                    if len({r[3] for r in g}) != 1 or len({r[5] for r in g}) != 1 or g[0][5] + sum(r[4] for r in g) != g[0][3]:
                        bad = True
                        continue
                    counts = {}
                    for r in g:
                        counts[r[2]] = counts.get(r[2], 0) + r[4]
                    agg[s][key] = (counts, g[0][3], g[0][1])
            if bad:
                dropped += 1
                continue
            for key in sorted(k for k in agg[0] if k in agg[1]):
                (ac, at, strand), (bc, bt, _) = agg[0][key], agg[1][key]
                pm = pmap(sum(ac.values()), at, sum(bc.values()), bt, prior, delta, max_coverages)
                ratio = pair.llk_ratio(ac, at, bc, bt)
                if pm is None or ratio is None:
                    failures += 1
                    continue
                sites.append({"chrom": key[0], "pos": key[1], "strand": strand, "a": (ac, at), "b": (bc, bt), "score": ratio[0], "terms": ratio[1],
                              "pmap": pm})
    return {"sites": sites, "max_coverages": max_coverages, "n_sampled": n_sampled, "n_batches": n_batches, "n_batches_dropped": dropped,
            "n_model_failures": failures}


HEADER = "\t".join(["chrom", "start", "end", "name", "score", "strand", "a_counts", "a_total", "b_counts", "b_total", "a_mod_percentages",
                    "b_mod_percentages", "a_pct_modified", "b_pct_modified", "map_pvalue", "effect_size"]) + "\n"


def f64_display(x):
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return pair.f64_display(x)


def site_fields(site):
    """the 16 fields of a site's row; score, map_pvalue and effect_size stay floats"""
    (ac, at), (bc, bt) = site["a"], site["b"]
    with np.errstate(all="ignore"):
        pa, pb = np.float32(sum(ac.values())) / np.float32(at), np.float32(sum(bc.values())) / np.float32(bt)
    return [site["chrom"], str(site["pos"]), str(site["pos"] + 1), ".", site["score"], site["strand"], pair.counts_text(ac), str(at),
            pair.counts_text(bc), str(bt), pair.counts_text(ac, at), pair.counts_text(bc, bt), pair.f32_display(pa), pair.f32_display(pb),
            site["pmap"]["p"], site["pmap"]["effect"]]


def table_text(sites, header=False):
    return (HEADER if header else "") + "".join("\t".join(f64_display(f) if isinstance(f, float) else f for f in site_fields(s)) + "\n" for s in sites)
