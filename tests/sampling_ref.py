"""Float64 reference of the on-device sampler's contract (penalty -> top-k ->
top-p -> seeded Gumbel-argmax; include/cake_hip.h, cake_hip_set_sampling_ex),
written from the contract and independent of cake_amd.serve, plus a numpy
restatement of the project's splitmix64 uniform stream.

Everything that decides the kept set is exact: the penalty is one f32
multiply, the order is the order of f32 values, ties are kept whole, so
`kept` and `tau` are compared with == against the device.  Only the top-p
boundary depends on rounding (masses, their sum); the test cases keep a
2^-10 margin of renormalised mass on both sides of it (tests/sampling_cases).

`mut` switches on one deliberate defect at a time; the CPU tests prove that
the cases notice each of them.
"""
import numpy as np

MUTATIONS = ("k_minus", "k_plus", "prefix_short", "prefix_long", "renorm_all",
             "sign_blind", "dup_twice", "bad_key")

_GOLD = np.uint64(0x9e3779b97f4a7c15)
_M1 = np.uint64(0xbf58476d1ce4e5b9)
_M2 = np.uint64(0x94d049bb133111eb)


K_MAX = (1 << 24) - 2        # the clamp of the top 24 hash bits


def u_of_hash(z):
    """The contract: k = top 24 bits of the hash,
    u = (min(k, 2^24 - 2) + 1) * 2^-24, worked from the integer k in float64.
    u lies in [2^-24, 1 - 2^-24]; every value is exact in float32."""
    k = np.minimum((z >> np.uint64(40)).astype(np.int64), K_MAX)
    u = (k + 1).astype(np.float64) * 2.0 ** -24
    assert ((u > 0) & (u < 1)).all()
    return u


def hash64(base, i1):
    """splitmix64 finaliser of base + M1 * i1 (uint64 arrays, wrapping)."""
    with np.errstate(over="ignore"):
        z = base + _M1 * i1
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def uniform_stream(seed, draw, V):
    """u_i in (0,1) for i < V at draw index `draw`: splitmix64 of
    seed + GOLD * (draw + 1) + M1 * (i + 1), top 24 bits clamped to 2^24 - 2,
    plus one, times 2^-24 (float64 holding f32-exact values)."""
    with np.errstate(over="ignore"):
        base = np.uint64(seed) + _GOLD * np.uint64(draw + 1)
    return u_of_hash(hash64(base, np.arange(1, V + 1, dtype=np.uint64)))


def uniform_at(seed, draws, ids):
    """The same stream at draw indices `draws` x vocabulary ids `ids` only
    (len(draws), len(ids)) — for draws over a small kept set."""
    d = np.asarray(draws, dtype=np.uint64)[:, None]
    i = np.asarray(ids, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        base = np.uint64(seed) + _GOLD * (d + np.uint64(1))
    return u_of_hash(hash64(base, i + np.uint64(1)))


def draws_on_support(lp, ids, temperature, seed, first, n):
    """Reference tokens of n consecutive draws when the kept set is `ids`
    (ascending): float64 Gumbel-argmax, first index on ties."""
    ids = np.asarray(ids)
    u = uniform_at(seed, np.arange(first, first + n), ids).astype(np.float64)
    v = np.asarray(lp, dtype=np.float64)[ids][None, :] / float(temperature)
    return ids[np.argmax(v - np.log(-np.log(u)), axis=1)]


def gumbel(seed, draw, V):
    u = uniform_stream(seed, draw, V).astype(np.float64)
    return -np.log(-np.log(u))


def keys(x, mut=None):
    """Order-preserving u32 keys of f32 values (sign flip); -0.0 == +0.0."""
    x = np.asarray(x, dtype=np.float32) + np.float32(0.0)  # -0 -> +0
    u = x.view(np.uint32)
    neg = (u & np.uint32(0x80000000)) != 0
    if mut == "bad_key":  # flips the sign bit only: negatives run backwards
        return u ^ np.uint32(0x80000000)
    return np.where(neg, ~u, u | np.uint32(0x80000000))


def penalise(logits, penalty, history, last_n=None, mut=None):
    """l' (float32).  history: previously sampled ids, oldest first."""
    lp = np.array(logits, dtype=np.float32)
    hist = [int(h) for h in history]
    if last_n is not None:
        hist = hist[-last_n:] if last_n > 0 else []
    if penalty == 1 or not hist:
        return lp
    ids = hist if mut == "dup_twice" else sorted(set(hist))
    inv = np.float32(1.0) / np.float32(penalty)
    pen = np.float32(penalty)
    for i in ids:
        v = lp[i]
        if mut == "sign_blind" or v >= 0:
            lp[i] = v * inv
        else:
            lp[i] = v * pen
    return lp


def select(lp, temperature, top_k=0, top_p=1.0, mut=None):
    """Kept set of penalised logits lp: dict(mask, kept, tau, before, upto)
    where before/upto are the renormalised cumulative masses just before and
    including the top-p boundary element (None when top-p is off)."""
    lp = np.asarray(lp, dtype=np.float32)
    V = lp.size
    key = keys(lp, mut).astype(np.int64)
    order = np.argsort(-key, kind="stable")
    skey = key[order]
    n = V
    bkey = skey[V - 1]
    k = int(top_k)
    if 0 < k < V and temperature > 0:
        if mut == "k_minus":
            k = max(1, k - 1)
        if mut == "k_plus":
            k = min(V, k + 1)
        bkey = skey[k - 1]
        n = int(np.sum(key >= bkey))
    before = upto = None
    if 0 < top_p < 1 and temperature > 0:
        x = lp[order].astype(np.float64)
        mx = x[0]
        with np.errstate(invalid="ignore"):
            d = np.where(x == mx, 0.0, x - mx)
        m = np.exp(d / float(temperature))
        total = m.sum() if mut == "renorm_all" else m[:n].sum()
        c = np.cumsum(m[:n]) / total
        j = min(int(np.searchsorted(c, top_p, side="left")), n - 1)
        if mut == "prefix_short":
            j = max(0, j - 1)
        if mut == "prefix_long":
            j = min(n - 1, j + 1)
        before = float(c[j - 1]) if j > 0 else 0.0
        upto = float(c[j])
        bkey = skey[j]
        n = int(np.sum(key >= bkey))
    mask = key >= bkey
    tau = lp[order[n - 1]] + np.float32(0.0)
    return dict(mask=mask, kept=n, tau=np.float32(tau), before=before,
                upto=upto)


def sample_ref(logits, temperature, top_k=0, top_p=1.0, penalty=1.0,
               history=(), last_n=None, mut=None):
    lp = penalise(logits, penalty, history, last_n, mut)
    out = select(lp, temperature, top_k, top_p, mut)
    out["lp"] = lp
    return out


def greedy_token(lp):
    """First-index argmax (what temperature <= 0 returns)."""
    return int(np.argmax(np.asarray(lp, dtype=np.float32)))


def draw_ref(lp, mask, temperature, seed, draw):
    """The reference draw in float64 (first index on ties).  The device
    computes the same expression in f32 with fast logs, so single tokens may
    differ on near-ties; distributions and supports may not."""
    lp = np.asarray(lp, dtype=np.float64)
    v = np.where(mask, lp / float(temperature) + gumbel(seed, draw, lp.size),
                 -np.inf)
    return int(np.argmax(v))


def chi_square(tokens, support, probs):
    """Pearson chi-square of `tokens` against `probs` on `support`; tokens
    outside the support count as an infinite statistic."""
    tokens = np.asarray(tokens)
    n = tokens.size
    stat = 0.0
    seen = 0
    for s, p in zip(support, probs):
        o = int(np.sum(tokens == s))
        seen += o
        stat += (o - n * p) ** 2 / (n * p)
    return stat if seen == n else float("inf")
