"""An independent f32 model of the reference's threshold caller, for the truth-table tests (tests/caller_truth_cases.py).

Pure Python + numpy float32; it imports neither the oracle nor modkit_amd.  Each function restates the reference source it cites,
in the reference's operation order, vectorised over calls: a map of k codes is an (n, k) float32 array whose column order is the
map's iteration order.

The reference keeps a call's probabilities in an FxHashMap and sums them in its iteration order, which this model does not restate.
`evaluate` runs the pipeline under every iteration order (of the map before and after the ReDistribute collapse): where all orders
agree the answer is the expectation, where they disagree the call is order-dependent (ties between two codes, or the rounded share of
a collapse over three codes) and `evaluate` says so.
"""
import itertools

import numpy as np

F32 = np.float32
MAX_PROB = F32(1.01)   # mod_bam.rs:26

# call classes
FILTERED, CANONICAL = -2, -1   # >= 0: Modified(code index)


def quals_to_probs(q):
    """quals_to_probs (mod_bam.rs:808-816): (qual + 0.5f32) / 256f32."""
    return (np.asarray(q, dtype=F32) + F32(0.5)) / F32(256)


def f32_sum(cols):
    """`values().sum::<f32>()` over the columns in iteration order (a left fold)."""
    s = np.zeros(cols[0].shape, dtype=F32) if cols else F32(0)
    for c in cols:
        s = (s + c).astype(F32)
    return s


def combine_fails(tag_probs, order):
    """combine_checked (mod_bam.rs:629-656) over the tags of one base in tag order: after each tag but the first is added, check()
    sums the map in `order` (code indices; codes not yet inserted are skipped) and fails when the sum exceeds MAX_PROB.
    tag_probs: list of (code indices of the tag, (n, len) float32).  Returns a bool array: the read fails at this call."""
    n = tag_probs[0][1].shape[0]
    have = {}
    bad = np.zeros(n, dtype=bool)
    for t, (codes, P) in enumerate(tag_probs):
        for j, c in enumerate(codes):
            have[c] = (have[c] + P[:, j]).astype(F32) if c in have else P[:, j]   # entry(..).or_insert(0) += prob
        if t > 0:
            bad |= f32_sum([have[c] for c in order if c in have]) > MAX_PROB   # check(): x > MAX_PROB
    return bad


def redistribute(P, order, x):
    """CollapseMethod::ReDistribute(x) of into_collapsed (mod_bam.rs:558-600).  P: (n, k); order: iteration order of the map.
    Returns (codes of the new map in the order they were inserted, (n, k') float32)."""
    marginal = f32_sum([P[:, c] for c in order if c == x])           # filter_map(code == x).sum()
    other = [c for c in order if c != x]
    n_other = F32(len(other)) + F32(1)                               # other_mods.len() as f32 + 1f32
    share = (marginal / n_other).astype(F32)
    return other, np.stack([(P[:, c] + share).astype(F32) for c in other], axis=1) if other else np.zeros((P.shape[0], 0), F32)


def call(P, order, thr_mod, thr_can):
    """MultipleThresholdModCaller::call (threshold_mod_caller.rs:28-63): the codes passing their threshold in iteration order, then
    Canonical(1 - sum) when it passes the canonical threshold, pushed last; `max()` under BaseModCall's PartialOrd (mod_bam.rs:379-397,
    by probability) returns the LAST maximum.  thr_mod[c]: the threshold of code column c.  Returns (class, probability)."""
    n = P.shape[0]
    cls = np.full(n, FILTERED, dtype=np.int64)
    best = np.zeros(n, dtype=F32)
    for c in order:
        p = P[:, c]
        take = (p >= thr_mod[c]) & ((cls == FILTERED) | ~(p < best))   # Iterator::max: a later equal element replaces the max
        cls = np.where(take, c, cls)
        best = np.where(take, p, best).astype(F32)
    pc = np.broadcast_to(F32(1) - f32_sum([P[:, c] for c in order]), (n,)).astype(F32)   # canonical_prob (mod_bam.rs:507-509)
    take = (pc >= thr_can) & ((cls == FILTERED) | ~(pc < best))
    return np.where(take, CANONICAL, cls), np.where(take, pc, best).astype(F32)


def argmax_call(P, order):
    """argmax_base_mod_call (mod_bam.rs:489-505): max_by(partial_cmp) keeps the last maximum; Modified only when strictly above the
    canonical probability.  Returns (class, probability)."""
    n = P.shape[0]
    pc = np.broadcast_to(F32(1) - f32_sum([P[:, c] for c in order]), (n,)).astype(F32)
    if not order:
        return np.full(n, CANONICAL, dtype=np.int64), pc
    bk = np.full(n, order[0], dtype=np.int64)
    best = P[:, order[0]]
    for c in order[1:]:
        p = P[:, c]
        take = ~(p < best)
        bk = np.where(take, c, bk)
        best = np.where(take, p, best).astype(F32)
    mod = best > pc
    return np.where(mod, bk, CANONICAL), np.where(mod, best, pc).astype(F32)


def percentile_linear_interp(xs, q):
    """percentile_linear_interp (thresholds.rs:17-38) on a sorted f32 sample."""
    xs = np.asarray(xs, dtype=F32)
    q = F32(q)
    assert len(xs) >= 2 and q <= F32(1)
    if q == F32(1):
        return xs[-1]
    l = F32(len(xs) - 1)
    lq = (l * q).astype(F32) if isinstance(l * q, np.ndarray) else F32(l * q)
    left, right = int(np.floor(lq)), int(np.ceil(lq))
    g = F32(lq - F32(np.floor(lq)))                                  # fract()
    return F32(F32(xs[left] * F32(F32(1) - g)) + F32(xs[right] * g))


def thresholds_for(codes, base, default, per_base=None, per_mod=None):
    """The threshold of each code (threshold_mod_caller.rs:36-43: per-mod, then the any-mod code of the base, then per-base, then the
    default) and the canonical threshold (l. 52-55: per-base, then the default)."""
    per_base, per_mod = per_base or {}, per_mod or {}

    def look(c):
        for v in (per_mod.get(c), per_mod.get(base), per_base.get(base)):
            if v is not None:
                return F32(v)
        return F32(default)
    return [look(c) for c in codes], F32(per_base.get(base, default))


def evaluate(codes, P, base="C", default=0.0, per_base=None, per_mod=None, collapse=None):
    """The threshold call and the argmax call of every call of one map layout, under every iteration order.
    codes: the code names of P's columns; collapse: the name of the code --ignore removes (ReDistribute) or None.
    Returns dict: cls (int64, code index into `out_codes` / CANONICAL / FILTERED), argmax_cls, argmax_p (float32), order_dep (bool),
    out_codes (the codes of the map the caller sees)."""
    k = len(codes)
    x = codes.index(collapse) if collapse in codes else None
    results = []
    for order in itertools.permutations(range(k)):
        if collapse is not None:
            other, Q = redistribute(P, list(order), x if x is not None else -1)
            names = [codes[c] for c in other]
        else:
            Q, names = P[:, list(order)], [codes[c] for c in order]
        thr, thr_can = thresholds_for(names, base, default, per_base, per_mod)
        for post in itertools.permutations(range(len(names))) if collapse is not None else [tuple(range(len(names)))]:
            c1, _ = call(Q, list(post), thr, thr_can)
            a1, ap = argmax_call(Q, list(post))
            # back to code names so that the orders compare
            m = np.array([codes.index(nm) for nm in names] + [0], dtype=np.int64)
            c1 = np.where(c1 >= 0, m[np.maximum(c1, 0)], c1)
            a1 = np.where(a1 >= 0, m[np.maximum(a1, 0)], a1)
            results.append((c1, a1, ap.view(np.uint32)))
    c0, a0, p0 = results[0]
    dep = np.zeros(P.shape[0], dtype=bool)
    for c1, a1, p1 in results[1:]:
        dep |= (c1 != c0) | (a1 != a0) | (p1 != p0)
    out_codes = [c for c in codes if c != collapse] if collapse is not None else list(codes)
    return dict(cls=c0, argmax_cls=a0, argmax_p=p0.view(F32), order_dep=dep, out_codes=out_codes)


def shortest(x):
    """The shortest positional decimal that reads back as the same f32 (numpy's repr; what Rust's `{}` prints for an f32)."""
    x = F32(x)
    if x == 0:
        return "-0" if np.signbit(x) else "0"
    s = np.format_float_positional(x, unique=True, trim="-")
    return s
