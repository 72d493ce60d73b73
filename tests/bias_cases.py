"""Cases, seeded inputs, float64 references and mutants of the q|k|v projection
bias (qwen2), shared by the GPU op tests (test_bias_ops_gpu.py) and the CPU
teeth tests (test_bias_ref.py), so every teeth condition is checked on exactly
the inputs the GPU sees.

Store kernels (k_rope_store_prefill / k_rope_store_decode with a bias row):
the kernel computes float(raw) + bias[row] in f32 and then exactly what it did
before, so the reference is tests/attn_ref.kv_store_ref on raw + b.  Inputs
are built so that every raw + b is EXACT in f32 (raw bf16 with |raw| in
[2^-6, 8), bias bf16 with |b| in [2^-6, 2^7]: all bits between 2^7 and 2^-13,
21 of f32's 24): V and V^T must then be RNE_bf16(raw + b) bit for bit, and q
and K stay inside kv_store_ref's bound.  The issue grants another
2^-24 (|x1| + |x2|) for the one f32 add; it is part of the bound here although
these inputs do not need it.

Fused kernel (k_gemv_qkv_rope_bias): tests/linear_ref's xhat and the formulas
of its qkv_rope_ref, with s + b in place of s, and |b| joining both bound
terms: mag is taken from the biased sums, acc from A + |b|.  Exact family:
the inputs of linear_cases.rope_inputs (every sum a multiple of 1/2 below
2^9) and a bias of +-2^j, j in [-2, 6], so every s + b is exact in f32 and V
is RNE_bf16(s + b) bit for bit; q and k pass through the f32 rotation by
irrational cos/sin and are held to rope_bound, as in test_qkv_rope.

Mutants are defects of how the bias row is indexed or applied; each is a
transformation of the bias row, except "after_rotation"."""
import numpy as np

from tests import linear_cases as lc
from tests import linear_ref as lr
from tests.attn_ref import kv_store_ref

STORE_MAX_SEQ = 64
STORE_GEOM = ((2, 1, 64), (4, 2, 128), (7, 1, 128), (14, 2, 64))
STORE_S = (1, 5, 33)
STORE_POS0 = (0, 7)
STORE_DECODE_POS = (0, 45, 63)
STORE_FAMILIES = ("wide", "large")
STALE = 2.0 ** 60
EPS = 1e-6

MUTANTS = ("q_dropped", "k_dropped", "v_dropped", "after_rotation", "shift_1",
           "shift_half", "shift_head", "kv_swapped", "q_neighbour_group")


def store_cases():
    """(nh, nkv, hd, S, pos0, decode)."""
    out = []
    for g in STORE_GEOM:
        out += [g + (S, p, False) for S in STORE_S for p in STORE_POS0]
        out += [g + (1, p, True) for p in STORE_DECODE_POS]
    return out


def fused_cases():
    """linear_cases.rope_cases() (KB 1, 2, 4, 8) and the two qwen2.5 head
    geometries at their real hidden sizes (KB 1, 2)."""
    out = list(lc.rope_cases())
    for i, g in enumerate(((7, 1, 128), (14, 2, 64))):
        for j, K in enumerate((896, 3584)):
            out.append(g + (K, lc.ROPE_POS[(i + j + 1) % 3]))
    return out


# ---- the bias row and its defects -------------------------------------------
def mutate_bias(b, mut, nh, nkv, hd):
    """The bias row a kernel with defect `mut` would effectively add, or None
    when the defect does not apply to (or changes nothing at) this shape."""
    b = np.asarray(b, dtype=np.float64)
    sq, skv = nh * hd, nkv * hd
    m = b.copy()
    if mut == "q_dropped":
        m[:sq] = 0
    elif mut == "k_dropped":
        m[sq:sq + skv] = 0
    elif mut == "v_dropped":
        m[sq + skv:] = 0
    elif mut == "shift_1":
        m = np.roll(b, 1)
    elif mut == "shift_half":              # the rope partner's value
        m = np.roll(b, hd // 2)
    elif mut == "shift_head":
        m = np.roll(b, hd)
    elif mut == "kv_swapped":
        m[sq:sq + skv], m[sq + skv:] = b[sq + skv:], b[sq:sq + skv]
    elif mut == "q_neighbour_group":       # q head h reads head h + nh/nkv
        if nkv < 2:
            return None
        m[:sq] = np.roll(b[:sq], -(nh // nkv) * hd)
    elif mut not in (None, "after_rotation"):
        raise KeyError(mut)
    return m


def _images(rng, nkv, max_seq, hd):
    """Cache images of ordinary values with +-2^60 mixed in; vtc is NOT the
    transpose of vc, so a write to a wrong column cannot hide."""
    def sentinel():
        a = rng.standard_normal((nkv, max_seq, hd))
        a = np.where(rng.random(a.shape) < 0.25,
                     rng.choice([-STALE, STALE], size=a.shape), a)
        return lc._q(a)
    return sentinel(), sentinel(), np.ascontiguousarray(
        sentinel().transpose(0, 2, 1))


# ---- store kernels ----------------------------------------------------------
def store_inputs(fam, nh, nkv, hd, S, pos0, decode):
    rng = lc._rng("bias_store", fam, nh, nkv, hd, S, pos0, decode)
    Nq = (nh + 2 * nkv) * hd
    max_seq = STORE_MAX_SEQ
    raw = 1.5 * rng.standard_normal((S, Nq))
    raw = lc._q(np.sign(raw) * np.clip(np.abs(raw), 2.0 ** -6, 7.875))
    lo = -6 if fam == "wide" else 3
    bias = lc._q(rng.choice([-1.0, 1.0], size=Nq) *
                 np.clip(2.0 ** rng.uniform(lo, 7, size=Nq), 2.0 ** -6,
                         2.0 ** 7))
    inv = 1.0 / np.power(10000.0, np.arange(0, hd, 2) / hd)
    ang = ((np.arange(max_seq)[:, None] + 0.5) * inv[None, :]).astype(
        np.float32)
    kc, vc, vtc = _images(rng, nkv, max_seq, hd)
    return dict(qkv=raw, bias=bias, cos=np.cos(ang), sin=np.sin(ang), kc=kc,
                vc=vc, vtc=vtc)


def store_ref(d, nh, nkv, hd, pos0, mut=None):
    """dict(q, qtol (S, nh, hd); kc, ktol, vc (nkv, max_seq, hd): K unrounded
    with its bound, V the unrounded raw + b), or None if mut does not apply."""
    b = mutate_bias(d["bias"], mut, nh, nkv, hd)
    if b is None:
        return None
    raw = d["qkv"].astype(np.float64)
    S = raw.shape[0]
    half = hd // 2
    if mut == "after_rotation":            # V has no rotation: unchanged
        pre = raw.copy()
        pre[:, (nh + nkv) * hd:] += b[(nh + nkv) * hd:]
    else:
        pre = raw + b
    q, kc, vc, _, qtol, ktol = kv_store_ref(pre, d["cos"], d["sin"], pos0, nh,
                                            nkv, d["kc"], d["vc"], d["vtc"])
    if mut == "after_rotation":
        q = q + b[:nh * hd].reshape(nh, hd)
        kc[:, pos0:pos0 + S] += b[nh * hd:(nh + nkv) * hd].reshape(
            nkv, 1, hd)
    # the one f32 add ahead of the rotation: 2^-24 (|x1| + |x2|)
    rows = pre.reshape(S, nh + 2 * nkv, hd)
    mag = np.abs(rows[..., :half]) + np.abs(rows[..., half:])
    add = 2.0 ** -24 * np.concatenate([mag, mag], axis=-1)
    qtol = qtol + add[:, :nh]
    ktol = ktol.copy()
    ktol[:, pos0:pos0 + S] += add[:, nh:nh + nkv].transpose(1, 0, 2)
    return dict(q=q, qtol=qtol, kc=kc, ktol=ktol, vc=vc)


def store_sums_exact(d):
    """Every raw + b of these inputs is exact in f32."""
    s32 = d["qkv"].astype(np.float32) + d["bias"].astype(np.float32)
    s64 = d["qkv"].astype(np.float64) + d["bias"].astype(np.float64)
    return bool((s32.astype(np.float64) == s64).all())


def store_moved(base, mutated, pos0, S):
    """A mutant moved q or K by more than twice the bound, or any V bit."""
    rows = slice(pos0, pos0 + S)
    if (np.abs(mutated["q"] - base["q"]) > 2 * base["qtol"]).any():
        return True
    if (np.abs(mutated["kc"][:, rows] - base["kc"][:, rows]) >
            2 * base["ktol"][:, rows]).any():
        return True
    return bool((lr.bf16_bits(mutated["vc"][:, rows]) !=
                 lr.bf16_bits(base["vc"][:, rows])).any())


# ---- fused kernel -----------------------------------------------------------
FUSED_FAMILIES = ("exact_dense", "random")


def fused_inputs(fam, nh, nkv, hd, K, pos):
    d = lc.rope_inputs(fam, nh, nkv, hd, K, pos)
    rng = lc._rng("bias_fused", fam, nh, nkv, hd, K, pos)
    Nq = (nh + 2 * nkv) * hd
    if d["exact"]:
        bias = rng.choice([-1.0, 1.0], size=Nq) * 2.0 ** rng.integers(
            -2, 7, size=Nq)
    else:                                  # q, k ~ N(0, 3); v ~ N(0, 0.25)
        bias = rng.standard_normal(Nq) * np.where(
            np.arange(Nq) < (nh + nkv) * hd, 3.0, 0.25)
    d["bias"] = bias.astype(np.float32)
    return d


def fused_ref(d, nh, nkv, hd, pos, mut=None):
    """dict(q, q_bound (nh, hd); k, k_bound (nkv, hd); v, v_bound (nkv, hd):
    v unrounded), or None if mut does not apply.  Bounds as in the module
    docstring."""
    b = mutate_bias(d["bias"], mut, nh, nkv, hd)
    if b is None:
        return None
    W = d["w"].astype(np.float64)
    xh = lr.xhat(d["x"], d["nw"], lc.EPS)
    s = W @ xh
    A = np.abs(W) @ np.abs(xh) + np.abs(b)
    nqk = (nh + nkv) * hd
    post = mut == "after_rotation"
    s = s + np.where(np.arange(s.size) < nqk, 0.0 if post else 1.0, 1.0) * b
    half = hd // 2
    c = np.asarray(d["cos"], np.float64)[pos]
    sn = np.asarray(d["sin"], np.float64)[pos]
    heads = s[:nqk].reshape(nh + nkv, hd)
    Ah = A[:nqk].reshape(nh + nkv, hd)
    lo, hi = heads[:, :half], heads[:, half:]
    roped = np.concatenate([lo * c - hi * sn, hi * c + lo * sn], axis=1)
    if post:
        roped = roped + b[:nqk].reshape(nh + nkv, hd)
    mag = np.concatenate([np.abs(lo * c) + np.abs(hi * sn),
                          np.abs(hi * c) + np.abs(lo * sn)], axis=1)
    acc = np.concatenate(
        [Ah[:, :half] * np.abs(c) + Ah[:, half:] * np.abs(sn),
         Ah[:, half:] * np.abs(c) + Ah[:, :half] * np.abs(sn)], axis=1)
    bound = lc.rope_bound(mag, acc)
    v = s[nqk:].reshape(nkv, hd)
    v_bound = (lc.TOL_BF16 * np.abs(v) + lc.TOL_F32 * A[nqk:].reshape(nkv, hd)
               + lc.ABS_EPS)
    return dict(q=roped[:nh], q_bound=bound[:nh], k=roped[nh:],
                k_bound=bound[nh:], v=v, v_bound=v_bound)


def fused_sums_exact(d, nh, nkv, hd, pos):
    """Exact family: every s + b is exact in f32."""
    xh = lr.xhat(d["x"], d["nw"], lc.EPS)
    s = d["w"].astype(np.float64) @ xh + d["bias"].astype(np.float64)
    return bool((s.astype(np.float32).astype(np.float64) == s).all() and
                (np.abs(np.abs(d["w"].astype(np.float64)) @ np.abs(xh)) +
                 np.abs(d["bias"]) < 2.0 ** 24).all())


def fused_moved(base, mutated, exact):
    for k in ("q", "k"):
        if (np.abs(mutated[k] - base[k]) > 2 * base[k + "_bound"]).any():
            return True
    if exact:
        return bool((lr.bf16_bits(mutated["v"]) !=
                     lr.bf16_bits(base["v"])).any())
    return bool((np.abs(mutated["v"] - base["v"]) >
                 2 * base["v_bound"]).any())
