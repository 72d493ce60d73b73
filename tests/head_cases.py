"""Cases, bounds, float64 references and mutant lists of the two ends of the
decode step: launch_argmax (greedy argmax, the plain-temperature Gumbel draw,
ring / step / pos bookkeeping), the Gumbel draw of launch_sample, and the
embedding gathers with the f32 <-> bf16 conversions.  Shared by the GPU tests
(test_head_ops_gpu.py) and the CPU teeth tests (test_head_ref.py), so every
teeth condition is checked on exactly the inputs the GPU sees.

The references are written from the contracts (DESIGN.md §7 item 3,
include/cake_hip.h):
  u       k = top 24 bits of splitmix64(seed + GOLD (draw + 1) + M1 (i + 1)),
          u = (min(k, 2^24 - 2) + 1) 2^-24, worked from the integer k
  argmax  the first index whose value equals the maximum over the non-NaN
          entries; 0 when no entry is greater than -inf; always < V
`mut` switches on one deliberate defect of the reference at a time.

Bounds (derived, not measured):
  Gumbel value  |G_dev - G_ref| <= 2^-18 (1 + |G_ref|): two f32 logs at about
          2^-22 relative error each (the inner one enters G absolutely, the
          outer one relatively), with 16x headroom.
  draw token    ref_score[tok] >= max(ref_score) - 2 tol, tol = 2^-18 (1 +
          |l| / T + |G|) at the reference maximum: the Gumbel bound plus the
          f32 roundings of 1 / T, l / T and the sum (3 * 2^-24 |l| / T).
  greedy, partials, bookkeeping, embedding rows: exact.
  nscale        relative TOL_F32 = 2^-16 (an f32 sum of H <= 16384 squares in
          a fixed tree of depth < 2^7, and rsqrtf)."""
import functools
import zlib

import numpy as np

from tests import linear_ref as lr
from tests import sampling_ref as sr

NPARTS = 256                 # launch_argmax: partitions == threads per block
BLOCK = 256
NONE = 0x7FFFFFFF            # "no index" of a span without a comparable value
SENT_BITS = 0xDD800000       # OP_SENTINEL (-2^60) as a 32-bit word
SENT_BF16 = 0xDD80
GUMBEL_TOL = 2.0 ** -18
TOL_F32 = 2.0 ** -16
EPS = 1e-5
K_TOP = (1 << 24) - 1

_M64 = (1 << 64) - 1
_GOLD, _M1, _M2 = 0x9e3779b97f4a7c15, 0xbf58476d1ce4e5b9, 0x94d049bb133111eb


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- the uniform stream, in Python integers ---------------------------------
def hash_k(seed, draw, i):
    """Top 24 bits of the hash at (seed, draw, vocabulary index i)."""
    z = (seed + _GOLD * (draw + 1) + _M1 * (i + 1)) & _M64
    z = ((z ^ (z >> 30)) * _M1) & _M64
    z = ((z ^ (z >> 27)) * _M2) & _M64
    return (z ^ (z >> 31)) >> 40


def gumbel_of_k(k):
    """float64 -log(-log(u)) at the contract's u of hash bits k."""
    u = (min(int(k), K_TOP - 1) + 1) * 2.0 ** -24
    return float(-np.log(-np.log(u)))


def gumbel_bound(g):
    return GUMBEL_TOL * (1.0 + np.abs(g))


# rows of (seed, draw, id) whose hash bits k are extreme; found by integer
# search over V = 8192, re-derived by test_head_ref.py
EXTREMES_V = 8192
EXTREMES = {
    K_TOP: ((2, 50, 5552), (4, 93, 5065), (1, 566, 3686)),
    K_TOP - 1: ((7, 160, 1216), (7, 750, 2938)),
    K_TOP - 2: ((4, 697, 3566), (4, 1369, 2892)),
    K_TOP - 3: ((1, 371, 1741), (6, 426, 5968)),
    0: ((5, 50, 883), (4, 230, 610)),
}
POISON_ROWS = EXTREMES[K_TOP]
PRODUCT_V = 151936
POISON_PRODUCT = (2, 41, 47740)            # k = 2^24 - 1 at the product vocab


def extreme_rows():
    return [(k, row) for k, rows in EXTREMES.items() for row in rows]


# ---- noise and scores (float64) ---------------------------------------------
def noise(seed, step, V, mut=None):
    """G_i for i < V at draw index `step`."""
    if mut == "step_off_by_one":
        step += 1
    i1 = np.arange(1, V + 1, dtype=np.uint64)
    if mut == "index_off_by_one":
        i1 = i1 - np.uint64(1)
    with np.errstate(over="ignore"):
        base = np.uint64(seed) + np.uint64(_GOLD) * np.uint64(step + 1)
    z = sr.hash64(base, i1)
    if mut == "u_can_be_one":              # no clamp: k = 2^24 - 1 -> u == 1
        u = ((z >> np.uint64(40)).astype(np.int64) + 1) * 2.0 ** -24
    else:
        u = sr.u_of_hash(z)
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(u))


def scores(logits, temperature, seed, step, mut=None):
    """l / T + G in float64 on the f32 logits (T <= 0: the logits)."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    if not temperature > 0:
        return l
    with np.errstate(invalid="ignore"):
        l = l * temperature if mut == "temp_multiplied" else l / temperature
        return l + noise(seed, step, l.size, mut)


# ---- argmax reference: partials and token -----------------------------------
def first_max(v, lo, hi, mut=None):
    """First index in [lo, hi) whose value equals the maximum over the
    non-NaN entries; NONE when there is none."""
    seg = v[lo:hi]
    nan = np.isnan(seg)
    if mut == "nan_wins" and nan.any():    # NaN compared as the largest
        return lo + int(np.argmax(nan))
    if seg.size == 0 or nan.all():
        return NONE
    eq = np.flatnonzero(seg == seg[~nan].max())
    return lo + int(eq[-1] if mut == "tie_last" else eq[0])


def spans(V, mut=None):
    """[start, end) of the 256 partitions."""
    span = V // NPARTS if mut == "span_floor" else (V + NPARTS - 1) // NPARTS
    out = []
    for p in range(NPARTS):
        s = min(p * span, V)
        e = min(s + span, V)
        if mut == "part_tail_dropped":     # the stride loop's remainder
            e = s + (e - s) // BLOCK * BLOCK
        out.append((s, e))
    return out


def argmax_ref(v, mut=None):
    """dict(token, pidx (256,) with NONE for spans without a winner) of
    values v (float64 or float32, NaN allowed)."""
    v = np.asarray(v)
    pidx = np.array([first_max(v, s, e, mut) for s, e in spans(v.size, mut)],
                    dtype=np.int64)
    pv = np.array([v[i] if i != NONE else -np.inf for i in pidx],
                  dtype=np.float64)
    n = NPARTS // 2 if mut == "fin_first_half_only" else NPARTS
    # spans are in index order: the first span holding the maximum holds the
    # first index (the last one under tie_last)
    j = first_max(pv, 0, n, mut)
    token = 0
    if j != NONE and pidx[j] != NONE and (
            pv[j] > -np.inf or (mut == "nan_wins" and np.isnan(pv[j]))):
        token = int(pidx[j])
    return dict(token=token, pidx=pidx)


def near_top(sc, tol_scale):
    """(ids with score >= max - 2 tol, max id, tol); tol = 2^-18 * tol_scale
    at the maximum."""
    i = int(np.argmax(sc))
    tol = GUMBEL_TOL * tol_scale[i]
    return np.flatnonzero(sc >= sc[i] - 2 * tol), i, tol


def draw_step_ref(logits, temperature, seed, step):
    """Reference of one Gumbel draw: dict(sc, near, top, tol)."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    g = noise(seed, step, l.size)
    sc = l / temperature + g
    near, top, tol = near_top(sc, 1.0 + np.abs(l) / temperature + np.abs(g))
    return dict(sc=sc, near=near, top=top, tol=tol)


# ---- greedy cases -----------------------------------------------------------
GREEDY_V = (1, 63, 255, 256, 257, 4099, 65537, 151936)


def span_of(V):
    return (V + NPARTS - 1) // NPARTS


def greedy_cases(V):
    """[(name, logits f32 (V,))]: every family of the issue that fits V."""
    rng = _rng("greedy", V)
    span = span_of(V)
    last_part = (V - 1) // span                # the last non-empty partition
    base = rng.standard_normal(V).astype(np.float32)
    out = []

    def add(name, x):
        out.append((name, np.asarray(x, dtype=np.float32)))

    def planted(ids, val=np.float32(9.0)):
        x = base.copy()
        x[list(ids)] = val
        return x
    pos = {"first": 0, "last": V - 1, "span-1": span - 1, "span": span,
           "lastpart_first": last_part * span}
    seen = set()
    for name, i in pos.items():
        if 0 <= i < V and i not in seen:
            seen.add(i)
            add(f"max@{name}", planted([i]))
    mid = (last_part // 2) * span              # first index of a middle span
    if span > BLOCK:                           # one thread's stride
        add("tie_stride", planted([mid, mid + BLOCK]))
    if span >= 2:                              # neighbouring threads
        add("tie_threads", planted([mid, mid + 1]))
    if last_part >= 1:                         # two partitions (both halves
        hi = last_part * span                  # of the final reduce)
        add("tie_parts", planted([span - 1, hi]))
        add("tie_parts_late", planted([hi - 1, V - 1]))
    add("all_equal", np.full(V, -3.25, dtype=np.float32))
    if V >= 2:
        x = -np.abs(base) - 1
        a, b = (span - 1, span) if span < V else (0, 1)
        x[a], x[b] = -0.0, 0.0
        add("negzero_first", x)
        x = base.copy()
        x[[V // 3, V - 1]] = np.inf
        add("inf_pair", x)
    add("all_neginf", np.full(V, -np.inf, dtype=np.float32))
    add("all_nan", np.full(V, np.nan, dtype=np.float32))
    if V >= 2:
        x = np.full(V, np.nan, dtype=np.float32)
        x[V // 2] = -7.5
        add("nan_but_one", x)
        x = np.full(V, -np.inf, dtype=np.float32)
        x[::2] = np.nan
        add("nan_neginf_mix", x)
        x = planted([V - 1])
        x[V // 2 - 1 if V > 2 else 0] = np.nan
        add("nan_before_max", x)
    return out


GREEDY_MUTANTS = ("tie_last", "span_floor", "part_tail_dropped",
                  "fin_first_half_only", "nan_wins")
GUMBEL_MUTANTS = ("u_can_be_one", "step_off_by_one", "index_off_by_one",
                  "temp_multiplied")
BOOK_MUTANTS = ("ring_at_zero",)
EMBED_MUTANTS = ("embed_row_next", "embed_tail_dropped", "nscale_no_eps",
                 "nscale_sum_not_mean")


# ---- bookkeeping ------------------------------------------------------------
BOOK_V, BOOK_T, BOOK_SEED = 4099, 1.0, 11
BOOK_FIRST, BOOK_STEPS = 3, 5


def book_logits():
    return _rng("book").standard_normal(BOOK_V).astype(np.float32)


def book_ref(tokens, first_step, ring, advance_pos, mut=None):
    """(ring image or None, step, pos) after len(tokens) launches."""
    n = len(tokens)
    if not ring:
        return None, first_step, n * advance_pos
    img = np.full(first_step + n, SENT_BITS, dtype=np.uint32)
    s = 0 if mut == "ring_at_zero" else first_step
    img[s:s + n] = tokens
    return img, first_step + n, n * advance_pos


# ---- Gumbel value, measured through one planted zero per partition ---------
GUMBEL_LOW = np.float32(-1e30)
SWEEP_V, SWEEP_SEED, SWEEP_DRAW = 4099, 3, 17
SWEEP_OFFSETS = (0, 5, 16)                 # index inside each 17-wide span


def planted_zero(V, ids):
    x = np.full(V, GUMBEL_LOW, dtype=np.float32)
    x[np.asarray(ids)] = 0.0
    return x


def sweep_ids(off):
    """One id per non-empty partition of SWEEP_V, `off` into its span."""
    return np.array([s + off for s, e in spans(SWEEP_V) if s + off < e])


# ---- poisoned token ---------------------------------------------------------
def poison_cases():
    """(V, seed, draw, id): the k = 2^24 - 1 rows, and the product vocab."""
    return [(EXTREMES_V,) + r for r in POISON_ROWS] + [
        (PRODUCT_V,) + POISON_PRODUCT]


def poison_logits(V, i):
    x = np.zeros(V, dtype=np.float32)
    x[i] = -1e4
    return x


# ---- draw tokens ------------------------------------------------------------
DRAW_STEPS = 64
# (V, T, seed, first step); seeds for which the near-top set is a single id in
# at least 99 % of the steps (test_head_ref.py checks it)
DRAW_CASES = ((4099, 0.7, 21, 0), (4099, 5.0, 22, 100),
              (PRODUCT_V, 0.7, 23, 7), (PRODUCT_V, 5.0, 24, 1000))


def draw_logits(V):
    return _rng("draw", V).standard_normal(V).astype(np.float32)


@functools.lru_cache(maxsize=None)
def draw_reference(V, T, seed, first):
    """Per step: (near-top ids, reference token, tol, reference scores are
    not kept: 64 x 151936 float64 is 78 MB)."""
    l = draw_logits(V)
    out = []
    for s in range(first, first + DRAW_STEPS):
        r = draw_step_ref(l, T, seed, s)
        out.append((r["near"], r["top"], r["tol"], float(r["sc"][r["top"]])))
    return out


# ---- embedding --------------------------------------------------------------
EMBED_H = (8, 72, 264, 4096, 16384)
EMBED_VT = 7
EMBED_BIG = (40, 16384)                    # > 2048 * 256: grid-stride loop
EDGE_ROW, ZERO_ROW = 1, 2
# f32 words and the bf16 words they must become (RNE; NaN -> 0x7fc0)
EDGE_WORDS = (
    (0x3F808000, 0x3F80),   # tie, even below: down
    (0x3F818000, 0x3F82),   # tie, odd below: up
    (0x3F808001, 0x3F81),   # just above a tie
    (0x3F817FFF, 0x3F81),   # just below a tie
    (0xBF818000, 0xBF82),
    (0x00000000, 0x0000), (0x80000000, 0x8000),
    (0x00000001, 0x0000),   # smallest f32 denormal
    (0x00030000, 0x0003),   # a bf16 denormal
    (0x00008000, 0x0000),   # denormal tie -> even
    (0x00018000, 0x0002),
    (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80),     # f32 max -> inf
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
    (0x7F800001, 0x7FC0),   # NaN, low payload
)


def embed_table(Vt, H):
    """f32 table (not bf16-exact: the upload has to round); row EDGE_ROW
    cycles through the conversion edges, row ZERO_ROW is zero."""
    t = _rng("embed", Vt, H).standard_normal((Vt, H)).astype(np.float32)
    w = np.array([a for a, _ in EDGE_WORDS], dtype=np.uint32)
    t[EDGE_ROW] = np.resize(w, H).view(np.float32)
    t[ZERO_ROW] = 0.0
    return t


def embed_ids(Vt, S):
    """0, Vt-1, a repeat, the edge and zero rows (S 5); the edge row (S 1)."""
    return np.array([EDGE_ROW] if S == 1 else
                    [0, Vt - 1, EDGE_ROW, Vt - 1, ZERO_ROW][:S],
                    dtype=np.uint32)


def embed_rows_cases():
    out = [(EMBED_VT, H, S) for H in EMBED_H for S in (1, 5)]
    return out + [EMBED_BIG + (5,)]


def embed_token_cases():
    """(Vt, H, id, with nscale)."""
    return [(EMBED_VT, H, i, ns) for H in EMBED_H
            for i in (0, EMBED_VT - 1, EDGE_ROW, ZERO_ROW)
            for ns in (False, True)]


def table_bits(t):
    # f32 max rounds to inf; widening a signalling NaN raises "invalid"
    with np.errstate(over="ignore", invalid="ignore"):
        return lr.bf16_bits(np.asarray(t, dtype=np.float32).astype(
            np.float64))


def embed_ref(table, ids, mut=None):
    """bf16 words (S, H) of the gathered rows; unwritten words hold the
    sentinel."""
    Vt, H = table.shape
    ids = np.asarray(ids, dtype=np.int64)
    if mut == "embed_row_next":
        ids = (ids + 1) % Vt
    out = table_bits(table)[ids]
    if mut == "embed_tail_dropped":
        out[:, H - 8:] = SENT_BF16
    return out


def nscale_ref(table, i, eps, mut=None):
    """float64 1 / sqrt(mean(x_bf16^2) + eps) of row i."""
    with np.errstate(over="ignore"):
        x = lr.bf16(table[i].astype(np.float64))
    ss = np.sum(x * x)
    m = ss if mut == "nscale_sum_not_mean" else ss / x.size
    with np.errstate(divide="ignore"):
        return 1.0 / np.sqrt(m + (0.0 if mut == "nscale_no_eps" else eps))
