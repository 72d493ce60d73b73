"""Deterministic cases for the sampler tests (CPU reference tests and GPU op
tests share them; the reference of each case is computed once and cached).

Logit families (f32, every value of the tail distinct so that top-k
boundaries are unambiguous unless a case ties them on purpose):
  peaky     five heavy tokens of both signs over a light tail
  plateau   up to 200 near-equal, strictly decreasing heavy tokens + tail
  negative  everything below zero
  mixed     heavy tokens straddling zero, one exactly 0.0
  neginf    peaky with a few -inf entries
  big       magnitudes up to 1e4 of both signs
  equal     all entries equal (the tie rule keeps everything)

top_p values are not free: each is placed halfway between the renormalised
cumulative masses before and including a chosen boundary token and is only
used when both gaps are >= MARGIN = 2^-10, four times the 2^-12 bound on
the device's mass accumulation error.  Boundary tokens therefore carry
>= 2^-9 of the mass, which is why deep cases are plateaus and not tails.
"""
import functools

import numpy as np

from tests.sampling_ref import penalise, sample_ref, select

MARGIN = 2.0 ** -10
VS = (1, 2, 63, 64, 65, 255, 1000, 4099, 128256, 151936)
FAMILIES = ("peaky", "plateau", "negative", "mixed", "neginf", "big", "equal")
T = 0.7
PENALTY = 1.3


def _tail(rng, n, lo, hi):
    """n distinct f32 values spread over [lo, hi) in random order."""
    if n <= 0:
        return np.zeros(0, dtype=np.float32)
    t = (lo + (hi - lo) * rng.permutation(n) / n).astype(np.float32)
    assert np.unique(t).size == n
    return t


@functools.lru_cache(maxsize=None)
def make_logits(family, V):
    """(logits f32 (V,), ids of the heavy tokens, heaviest first)."""
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + V % 997)
    if family == "equal":
        return np.full(V, 1.5, dtype=np.float32), np.arange(min(V, 4))
    if family == "peaky":
        heavy, lo, hi = [6.0, 5.1, 4.4, -0.5, -1.2], -19.0, -11.0
    elif family == "plateau":
        heavy = list(5.0 - 1e-3 * np.arange(200))
        lo, hi = -24.0, -14.0
    elif family == "negative":
        heavy = list(-20.0 - 0.6 * np.arange(8))
        lo, hi = -48.0, -38.0
    elif family == "mixed":
        heavy = [2.1, 1.4, 0.7, 0.0, -0.7, -1.4, -2.1]
        lo, hi = -22.0, -14.0
    elif family == "neginf":
        heavy, lo, hi = [3.0, 2.5, -0.25, -1.0], -19.0, -11.0
    elif family == "big":
        heavy = [1e4, 1e4 - 0.5, 1e4 - 1.25, 1e4 - 2.0]
        lo, hi = -1e4, 5e3
    else:
        raise ValueError(family)
    c = min(len(heavy), V)
    x = _tail(rng, V, lo, hi)
    ids = np.sort(rng.choice(V, size=c, replace=False))
    ids = ids[rng.permutation(c)]
    x[ids] = np.asarray(heavy[:c], dtype=np.float32)
    if family == "neginf":
        free = np.setdiff1d(np.arange(V), ids)
        x[free[:: max(1, free.size // 5)][:5]] = -np.inf
    return x, ids


def history_for(family, V):
    """Sampled-id history with duplicates, the ids 0 and V-1, and heavy
    tokens of both signs where the family has them."""
    _, ids = make_logits(family, V)
    h = [0, V - 1, int(ids[0]), int(ids[-1]), int(ids[0]), 0]
    h += [int(i) for i in ids[: min(4, len(ids))]]
    if len(ids) > 3:
        h += [int(ids[3]), int(ids[3])]
    return h


def pick_top_p(lp, temperature, top_k, depth):
    """top_p whose boundary is the depth-th survivor, or None when the
    margin cannot be met there."""
    V = lp.size
    k = top_k if 0 < top_k < V else V
    order = np.argsort(-lp.astype(np.float64), kind="stable")
    x = lp[order].astype(np.float64)
    n = int(np.sum(lp >= x[k - 1]))
    with np.errstate(invalid="ignore"):
        d = np.where(x[:n] == x[0], 0.0, x[:n] - x[0])
    m = np.exp(d / temperature)
    c = np.cumsum(m) / m.sum()
    j = min(depth, n - 1)
    before = c[j - 1] if j > 0 else 0.0
    p = 0.5 * (before + c[j])
    if p - before < MARGIN * 1.01 or c[j] - p < MARGIN * 1.01 or p >= 1:
        return None
    if j > 0 and x[j] == x[j - 1]:
        return None
    return float(p)


@functools.lru_cache(maxsize=None)
def cases(family, V):
    """List of dicts: name, mode ('k', 'p', 'kp'), top_k, top_p, penalty,
    history.  Same list for every consumer."""
    logits, _ = make_logits(family, V)
    out = []
    for pen in (1.0, PENALTY):
        hist = tuple(history_for(family, V)) if pen != 1.0 else ()
        lp = penalise(logits, pen, hist)
        tag = "+pen" if pen != 1.0 else ""
        for k in (1, 2, 40, V - 1, V, V + 7):
            out.append(dict(name=f"k{k}{tag}", mode="k", top_k=k, top_p=1.0,
                            penalty=pen, history=hist))
        for depth in (0, 1, 2, 3, 100, 199):
            p = pick_top_p(lp, T, 0, depth)
            if p is not None:
                out.append(dict(name=f"p@{depth}{tag}", mode="p", top_k=0,
                                top_p=p, penalty=pen, history=hist))
        for k, depth in ((3, 1), (40, 20), (40, 39), (2, 0)):
            p = pick_top_p(lp, T, k, depth)
            if p is not None:
                out.append(dict(name=f"k{k}p@{depth}{tag}", mode="kp",
                                top_k=k, top_p=p, penalty=pen, history=hist))
    return out


@functools.lru_cache(maxsize=None)
def reference(family, V, idx, mut=None):
    c = cases(family, V)[idx]
    logits, _ = make_logits(family, V)
    return sample_ref(logits, T, c["top_k"], c["top_p"], c["penalty"],
                      c["history"], mut=mut)


def tie_case(V):
    """top-k whose k-th value is shared by a group of 5: k = 3 lands inside
    the group, the whole group survives (kept = 6)."""
    rng = np.random.default_rng(77 + V)
    x = _tail(rng, V, -9.0, -3.0)
    ids = rng.choice(V, size=6, replace=False)
    x[ids[0]] = 4.0
    x[ids[1:]] = 2.5
    return x, 3, 6, np.float32(2.5)


def chi_case(V):
    """4-token support with masses .4/.3/.2/.1 at T (the tail is cut by
    top_k = 4), for the chi-square condition."""
    rng = np.random.default_rng(5 + V)
    x = _tail(rng, V, -30.0, -20.0)
    ids = np.sort(rng.choice(V, size=4, replace=False))
    probs = np.array([0.4, 0.3, 0.2, 0.1])
    x[ids] = (T * np.log(probs)).astype(np.float32)
    return x, ids, probs


__all__ = ["MARGIN", "VS", "FAMILIES", "T", "PENALTY", "make_logits",
           "history_for", "cases", "reference", "tie_case", "chi_case",
           "select"]
