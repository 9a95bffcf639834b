"""An independent model of `modkit dmr pair -a A1 -a A2 .. -b B1 -b B2 .. --ref ref.fa --base C` WITHOUT -r, with replicates (v0.4.4:
SingleSiteDmrAnalysis::run, SingleSiteDmrScore::new_multi / to_row / to_row_pair and collapse_counts in src/dmr/single_site.rs,
SingleSiteSampleIndex in src/dmr/tabix.rs, AggregatedCounts in src/dmr/llr_model.rs), written from those files and not from the library's
C++ or its kernels.  What replicates do not change (the row filter, the walk, the percentile, the p-value, the likelihood ratio) is
dmr_sites_model's and dmr_pair_model's; the f32 arithmetic of the balanced counts and of the shares of samples is numpy.float32, one
operation at a time; the extra columns have a text writer of their own.

One deliberate departure, as the library's: the present samples of a site are listed in ascending command-line index, where the
reference takes the iteration order of an FxHashMap<usize, _>."""
import math

import numpy as np

import dmr_pair_model as pair
import dmr_sites_model as sites

ModelError = sites.ModelError
F = np.float32


def multiple(n_a, n_b):
    return n_a > 1 or n_b > 1


def matched(n_a, n_b):
    return n_a == n_b and n_a > 1


def pct_samples(n_present, n):
    """((n_present as f32 / n as f32) * 100f32).floor() as usize"""
    return int(np.floor((F(n_present) / F(n)) * F(100)))


def cast_usize(x):
    """Rust's `f32 as usize`: NaN -> 0, saturating"""
    x = float(x)
    if x != x or x <= 0.0:
        return 0
    return 2 ** 64 - 1 if math.isinf(x) else min(int(x), 2 ** 64 - 1)


def balanced_one(counts, total, target):
    """one sample under collapse_counts(_, true): ({code: floor(count / total * target)}, target as usize)"""
    out = {}
    with np.errstate(all="ignore"):
        for code, c in counts.items():
            frac = F(c) / F(total)
            out[code] = cast_usize(np.floor(frac * target))
    return out, cast_usize(np.trunc(target))


def collapse(samples, balance):
    """collapse_counts: samples = [({code: n_mod}, total)] -> ({code: n_mod}, total, ok); ok = False where try_new(..).unwrap() would abort"""
    if len(samples) == 1:
        return dict(samples[0][0]), samples[0][1], True
    ok = True
    if balance:
        target = F(sum(t for _c, t in samples)) / F(len(samples))
        parts = [balanced_one(c, t, target) for c, t in samples]
        ok = all(sum(c.values()) <= t for c, t in parts)
    else:
        parts = samples
    counts, total = {}, 0
    for c, t in parts:
        for code, n in c.items():
            counts[code] = counts.get(code, 0) + n
        total += t
    return counts, total, ok


def collapse_f64(samples):
    """the balanced counts had the reference worked in f64: only to show that a test set tells the two apart"""
    if len(samples) == 1:
        return dict(samples[0][0]), samples[0][1]
    target = sum(t for _c, t in samples) / len(samples)
    counts = {}
    for c, t in samples:
        for code, n in c.items():
            counts[code] = counts.get(code, 0) + (int(math.floor(n / t * target)) if t else 0)
    return counts, int(target) * len(samples)


def score_site(a_samples, b_samples, n_a, n_b, prior, delta, max_coverages):
    """SingleSiteDmrScore::new_multi over the present samples (ascending index): a dict, or None where any evaluation fails"""
    reps = None
    if matched(n_a, n_b) and len(a_samples) == len(b_samples):
        reps = [sites.pmap(sum(ac.values()), at, sum(bc.values()), bt, prior, delta, max_coverages) for (ac, at), (bc, bt) in zip(a_samples, b_samples)]
        if any(r is None for r in reps):
            return None
    pct = (pct_samples(len(a_samples), n_a), pct_samples(len(b_samples), n_b))
    ba, bat, ok_a = collapse(a_samples, True)
    bb, bbt, ok_b = collapse(b_samples, True)
    if not (ok_a and ok_b):
        return None   # (the reference aborts here; the library counts a model failure)
    bal = sites.pmap(sum(ba.values()), bat, sum(bb.values()), bbt, prior, delta, max_coverages)
    if bal is None or pair.llk_ratio(ba, bat, bb, bbt) is None:
        return None
    ca, cat, _ = collapse(a_samples, False)
    cb, cbt, _ = collapse(b_samples, False)
    pm = sites.pmap(sum(ca.values()), cat, sum(cb.values()), cbt, prior, delta, max_coverages)
    ratio = pair.llk_ratio(ca, cat, cb, cbt)
    if pm is None or ratio is None:
        return None
    return {"a": (ca, cat), "b": (cb, cbt), "score": ratio[0], "terms": ratio[1], "pmap": pm, "balanced": bal, "bal_a": (ba, bat), "bal_b": (bb, bbt),
            "pct": pct, "reps": reps}


def run(tables_a, tables_b, fasta, bases=("C",), lookup=None, min_cov=0, mask=False, prior=(0.55, 0.55), delta=0.05, max_coverages=None,
        n_sample=10042, interval=100000, batch_size=6, cap_coverages=False):
    """The whole run: tables_a / tables_b = lists of record lists.  Returns dmr_sites_model.run's dict; a site also holds "balanced" (a pmap
    dict), "bal_a" / "bal_b", "pct" (a, b), "reps" (a list of pmap dicts, or None), "present" (a's indices, b's indices)."""
    lookup = sites.DEFAULT_LOOKUP if lookup is None else lookup
    n_a, n_b = len(tables_a), len(tables_b)
    tables = list(tables_a) + list(tables_b)
    side = [0] * n_a + [1] * n_b
    has = lambda n, sd: any(r[0] == n for t, s in zip(tables, side) if s == sd for r in t)
    contigs = sorted((n for n in fasta if has(n, 0) and has(n, 1)), key=lambda n: n.encode())
    if not contigs:
        raise ModelError("need at least 1 contig")
    listed, lengths = {}, {}
    for n in contigs:
        listed[n] = sites.listed_positions(fasta[n], bases, mask)
        listed[n + "#arr"] = np.array(sorted(listed[n]), dtype=np.int64)
        lengths[n] = len(fasta[n])
    part = [{n: [] for n in contigs} for _t in tables]
    for s, recs in enumerate(tables):
        for chrom, pos, code, strand, n_valid, n_mod, n_can in recs:
            if chrom not in part[s] or n_valid < min_cov or code not in lookup:
                continue
            st = "-" if strand == "-" else "+"
            base = pair.COMPLEMENT[lookup[code]] if st == "-" else lookup[code]
            if listed[chrom].get(pos) == (st, base):
                part[s][chrom].append((pos, st, code, n_valid, n_mod, n_can))
    supers = sites.super_batches(contigs, listed, lengths, interval, batch_size)

    n_sampled = (0, 0)
    if max_coverages is None:
        cov = [[], []]
        for sb in supers:
            for batch in sb:
                for s in range(len(tables)):
                    cov[side[s]] += [r[3] for chrom, lo, hi in batch for r in part[s][chrom] if lo <= r[0] < hi]
            if min(len(cov[0]), len(cov[1])) >= n_sample:
                break
        n_sampled = (len(cov[0]), len(cov[1]))
        max_coverages = tuple(int(np.floor(sites.percentile_linear_interp(sorted(np.float32(v) for v in c), 0.95))) for c in cov)
    # PMapEstimator::new: times the side's number of tables unless --cap-coverages, then the cap
    max_coverages = tuple(min(int(m) * (1 if cap_coverages else n), sites.MAX_COV_ALLOWED) for m, n in zip(max_coverages, (n_a, n_b)))

    out, dropped, failures, n_batches = [], 0, 0, 0
    for sb in supers:
        for batch in sb:
            n_batches += 1
            agg, bad = [{} for _t in tables], False
            for s in range(len(tables)):
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
            keys_a = set().union(*[set(agg[s]) for s in range(n_a)])
            keys_b = set().union(*[set(agg[s]) for s in range(n_a, n_a + n_b)])
            for key in sorted(keys_a & keys_b):
                pa = [s for s in range(n_a) if key in agg[s]]
                pb = [s - n_a for s in range(n_a, n_a + n_b) if key in agg[s]]
                res = score_site([agg[s][key][:2] for s in pa], [agg[n_a + s][key][:2] for s in pb], n_a, n_b, prior, delta, max_coverages)
                if res is None:
                    failures += 1
                    continue
                res.update({"chrom": key[0], "pos": key[1], "strand": agg[pa[0]][key][2], "present": (pa, pb)})
                out.append(res)
    return {"sites": out, "max_coverages": max_coverages, "n_sampled": n_sampled, "n_batches": n_batches, "n_batches_dropped": dropped,
            "n_model_failures": failures, "n_a": n_a, "n_b": n_b}


def evaluations(site):
    """every pmap dict of a site: collapsed, balanced, then the replicate pairs"""
    return [site["pmap"], site["balanced"]] + list(site["reps"] or [])


EXTRA_MULTIPLE = ["balanced_map_pvalue", "balanced_effect_size", "pct_a_samples", "pct_b_samples"]
EXTRA_MATCHED = ["replicate_map_pvalues", "replicate_effect_sizes"]


def header(n_a, n_b):
    fields = sites.HEADER.rstrip("\n").split("\t")
    if multiple(n_a, n_b):
        fields += EXTRA_MULTIPLE
    if matched(n_a, n_b):
        fields += EXTRA_MATCHED
    return "\t".join(fields) + "\n"


def site_fields(site, n_a, n_b):
    """the fields of a site's row; f64 values stay floats, a replicate list is a list of floats or the string `-`"""
    f = sites.site_fields(site)
    if multiple(n_a, n_b):
        f += [site["balanced"]["p"], site["balanced"]["effect"], str(site["pct"][0]), str(site["pct"][1])]
    if matched(n_a, n_b):
        f += [[r["p"] for r in site["reps"]], [r["effect"] for r in site["reps"]]] if site["reps"] else ["-", "-"]
    return f


def field_text(f):
    if isinstance(f, float):
        return sites.f64_display(f)
    if isinstance(f, list):
        return ",".join(sites.f64_display(x) for x in f)
    return f


def table_text(res, with_header=False):
    n_a, n_b = res["n_a"], res["n_b"]
    return (header(n_a, n_b) if with_header else "") + "".join("\t".join(field_text(f) for f in site_fields(s, n_a, n_b)) + "\n" for s in res["sites"])
