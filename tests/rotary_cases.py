"""Cases, seeded inputs, float64 references and defects of PARTIAL ROTARY (only
the first rd < hd dims of a q / k head rotate; phi3's partial_rotary_factor),
shared by the GPU op tests (test_rotary_ops_gpu.py) and the CPU teeth tests
(test_rotary_ref.py), so every teeth condition is checked on exactly the calls
the GPU makes.

Store kernels (k_rope_store_prefill / k_rope_store_decode with rd < hd): the
raw rows are bf16, so V, V^T, K's pass-through dims and q's (left in place) are
the raw bits; rotated dims carry tests/attn_ref.kv_store_ref's bound
(one bf16 ulp of the result + 2^-22 (|x1| + |x2|)).

Fused kernel (k_gemv_qkv_rope_pr): tests/linear_ref's xhat and the formulas of
its qkv_rope_ref, with the pairing (i, i + rd/2), i < rd/2.  Exact family (the
inputs of linear_cases.rope_inputs: every sum a multiple of 1/2 below 2^9):
pass-through dims and V are RNE_bf16 of the exact sum bit for bit, rotated dims
inside linear_cases.rope_bound.  Random family: rotated dims inside rope_bound,
pass-through dims and V inside 2^-8 |v| + 2^-16 A.

The tables are (max_seq, rd/2), rows differing at every position, 0 included.

Defects (DEFECTS) are ways a partial-rotary kernel goes wrong; `rotate` applies
one on purpose.  One that cannot show at a shape (no neighbouring head, pos 0
for the stride) yields None there."""
import functools

import numpy as np

from tests import linear_cases as lc
from tests import linear_ref as lr
from tests.attn_ref import bf16_ulp

STORE_MAX_SEQ = 64
STORE_GEOM = ((2, 1, 16, 12), (4, 2, 64, 48), (3, 1, 128, 96),
              (4, 1, 128, 32), (2, 1, 128, 4), (2, 1, 128, 124))
STORE_S = (1, 5, 33)
STORE_POS0 = (0, 7)
STORE_DECODE_POS = (0, 45, 63)
STALE = 2.0 ** 60
EPS = 1e-6
FUSED_FAMILIES = ("exact_dense", "random")

DEFECTS = ("pair_half_hd",          # pairs (i, i + hd/2) instead of rd/2
           "full_rotation",         # all hd dims rotate
           "pass_rotated_pair0",    # a pass block rotated with pair 0
           "pass_not_written",
           "pass_shift_half",       # pass dims read rd/2 lower
           "pass_shift_rest",       # ... hd - rd lower
           "table_stride_hd",       # table row stride hd/2
           "k_pass_neighbour_kv",   # k pass dims of kv head h + 1
           "q_pass_neighbour",      # q pass dims of head h + 1
           "v_col_off")             # V lands 4 columns off


def store_cases():
    """(nh, nkv, hd, rd, S, pos0, decode)."""
    out = []
    for g in STORE_GEOM:
        out += [g + (S, p, False) for S in STORE_S for p in STORE_POS0]
        out += [g + (1, p, True) for p in STORE_DECODE_POS]
    return out


def fused_cases():
    """(nh, nkv, hd, rd, K, pos): linear_cases.rope_cases() (KB 1, 2, 4, 8),
    each with rd in {3/4 hd, hd/4, 4, hd - 4}, and Phi-4-mini's head geometry
    at its hidden size."""
    out = []
    for nh, nkv, hd, K, pos in lc.rope_cases():
        for rd in (hd * 3 // 4, hd // 4, 4, hd - 4):
            out.append((nh, nkv, hd, rd, K, pos))
    out.append((24, 8, 128, 96, 3072, 45))
    return out


def tables(max_seq, rd):
    inv = 1.0 / np.power(10000.0, np.arange(0, rd, 2) / rd)
    ang = ((np.arange(max_seq)[:, None] + 0.5) * inv[None, :]).astype(
        np.float32)
    return np.cos(ang), np.sin(ang)


# ---- the rotation of one position, with an optional defect -------------------
def _tab(t, p, idx, hd, mut):
    t = np.asarray(t, dtype=np.float64)
    if mut == "table_stride_hd":
        return t.reshape(-1)[(p * (hd // 2) + idx) % t.size]
    return t[p, idx]


def rotate(rows, cos, sin, p, nh, nkv, hd, rd, mut=None, q_prior=None,
           k_prior=None):
    """rows (nh + 2*nkv, hd) float64: the values ahead of the rotation.
    Returns (qk (nh + nkv, hd) after it, v (nkv, hd), rot: which dims of qk
    are rotated, a1, a2: the two products summed in every rotated dim), or None when
    `mut` cannot show here.  q_prior / k_prior: what an unwritten q / k
    element holds ((nh, hd) / (nkv, hd))."""
    H = nh + nkv
    half = rd // 2
    if mut in ("k_pass_neighbour_kv",) and nkv < 2:
        return None
    if mut == "q_pass_neighbour" and nh < 2:
        return None
    if mut == "table_stride_hd" and p == 0:
        return None
    if mut == "pair_half_hd":
        n, part = half, hd // 2
    elif mut == "full_rotation":
        n, part = hd // 2, hd // 2
    else:
        n, part = half, half
    idx = np.arange(n) % half
    c, s = _tab(cos, p, idx, hd, mut), _tab(sin, p, idx, hd, mut)
    qk = rows[:H]
    out = qk.copy()
    x1, x2 = qk[:, :n], qk[:, part:part + n]
    out[:, :n] = x1 * c - x2 * s
    out[:, part:part + n] = x2 * c + x1 * s
    rot = np.zeros((H, hd), dtype=bool)
    rot[:, :n] = rot[:, part:part + n] = True
    a1 = np.zeros((H, hd))
    a2 = np.zeros((H, hd))
    a1[:, :n], a2[:, :n] = x1 * c, x2 * s
    a1[:, part:part + n], a2[:, part:part + n] = x2 * c, x1 * s
    if mut == "pass_rotated_pair0":
        c0, s0 = _tab(cos, p, np.arange(2), hd, mut), \
            _tab(sin, p, np.arange(2), hd, mut)
        for d0 in range(rd, hd, 4):
            lo, hi = qk[:, d0:d0 + 2], qk[:, d0 + 2:d0 + 4]
            out[:, d0:d0 + 2] = lo * c0 - hi * s0
            out[:, d0 + 2:d0 + 4] = hi * c0 + lo * s0
    elif mut == "pass_not_written":
        out[:nh, rd:] = q_prior[:, rd:]
        out[nh:, rd:] = k_prior[:, rd:]
    elif mut in ("pass_shift_half", "pass_shift_rest"):
        shift = half if mut == "pass_shift_half" else hd - rd
        flat = rows.reshape(-1)
        src = (np.arange(H)[:, None] * hd + np.arange(rd, hd)[None, :] -
               shift) % flat.size
        out[:, rd:] = flat[src]
    elif mut == "k_pass_neighbour_kv":
        out[nh:, rd:] = np.roll(qk[nh:, rd:], -1, axis=0)
    elif mut == "q_pass_neighbour":
        out[:nh, rd:] = np.roll(qk[:nh, rd:], -1, axis=0)
    v = rows[H:]
    if mut == "v_col_off":
        v = np.roll(v, 4, axis=1)
    return out, v, rot, a1, a2


# ---- store kernels ----------------------------------------------------------
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


def store_inputs(nh, nkv, hd, rd, S, pos0, decode):
    rng = lc._rng("rotary_store", nh, nkv, hd, rd, S, pos0, decode)
    Nq = (nh + 2 * nkv) * hd
    raw = lc._q(1.5 * rng.standard_normal((S, Nq)))
    cos, sin = tables(STORE_MAX_SEQ, rd)
    kc, vc, vtc = _images(rng, nkv, STORE_MAX_SEQ, hd)
    return dict(qkv=raw, cos=cos, sin=sin, kc=kc, vc=vc, vtc=vtc)


def store_ref(d, nh, nkv, hd, rd, pos0, mut=None):
    """dict(q, qtol, qrot (S, nh, hd); kc, ktol, krot, vc (nkv, max_seq, hd)):
    unrounded values, the bound of the rotated dims (elsewhere the value is a
    bf16 the kernel must reproduce bit for bit), or None if `mut` cannot show
    at any row of this call."""
    raw = d["qkv"].astype(np.float64)
    S = raw.shape[0]
    kc = np.array(d["kc"], dtype=np.float64)
    vc = np.array(d["vc"], dtype=np.float64)
    q = np.empty((S, nh, hd))
    qtol = np.zeros((S, nh, hd))
    qrot = np.zeros((S, nh, hd), dtype=bool)
    ktol = np.zeros_like(kc)
    krot = np.zeros(kc.shape, dtype=bool)
    shown = False
    for i in range(S):
        p = pos0 + i
        rows = raw[i].reshape(nh + 2 * nkv, hd)
        r = rotate(rows, d["cos"], d["sin"], p, nh, nkv, hd, rd, mut,
                   q_prior=rows[:nh], k_prior=kc[:, p])
        if r is None:                    # cannot show at this row
            r = rotate(rows, d["cos"], d["sin"], p, nh, nkv, hd, rd)
        else:
            shown = True
        out, v, rot, a1, a2 = r
        # kv_store_ref's bound, from the rotation's own inputs
        tol = bf16_ulp(out) + 2.0 ** -22 * _pair_mag(rows[:nh + nkv], rot, rd)
        q[i], qtol[i], qrot[i] = out[:nh], tol[:nh], rot[:nh]
        kc[:, p], ktol[:, p], krot[:, p] = out[nh:], tol[nh:], rot[nh:]
        vc[:, p] = v
    if mut is not None and not shown:
        return None
    return dict(q=q, qtol=qtol, qrot=qrot, kc=kc, ktol=ktol, krot=krot, vc=vc)


def _pair_mag(qk, rot, rd):
    """|x1| + |x2| of the correct pairing, at both dims of every pair."""
    half = rd // 2
    m = np.zeros_like(qk)
    pm = np.abs(qk[:, :half]) + np.abs(qk[:, half:rd])
    m[:, :half] = m[:, half:rd] = pm
    return m


def store_moved(base, mutated, pos0, S):
    """A defect moved a rotated q / K dim by more than twice the bound, or any
    bit of a pass-through dim or of V."""
    rows = slice(pos0, pos0 + S)
    for a, tol, rot in (("q", "qtol", "qrot"), ("kc", "ktol", "krot")):
        b, m = base[a], mutated[a]
        t, r = base[tol], base[rot]
        if a == "kc":
            b, m, t, r = b[:, rows], m[:, rows], t[:, rows], r[:, rows]
        if (np.abs(m - b)[r] > 2 * t[r]).any():
            return True
        if (lr.bf16_bits(m[~r]) != lr.bf16_bits(b[~r])).any():
            return True
    return bool((lr.bf16_bits(mutated["vc"][:, rows]) !=
                 lr.bf16_bits(base["vc"][:, rows])).any())


# ---- fused kernel -----------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _fused_base(fam, nh, nkv, hd, K, pos):
    """linear_cases.rope_inputs and the float64 sums, shared by the rd values
    of one geometry (the tables are the only input that depends on rd)."""
    d = lc.rope_inputs(fam, nh, nkv, hd, K, pos)
    W = d["w"].astype(np.float64)
    xh = lr.xhat(d["x"], d["nw"], lc.EPS)
    d["s"] = W @ xh
    d["A"] = np.abs(W) @ np.abs(xh)
    return d


def fused_inputs(fam, nh, nkv, hd, rd, K, pos):
    d = dict(_fused_base(fam, nh, nkv, hd, K, pos))
    d["cos"], d["sin"] = tables(lc.ROPE_MAX_SEQ, rd)
    return d


def fused_ref(d, nh, nkv, hd, rd, pos, mut=None, q_prior=None):
    """dict(q, k, v: unrounded (heads, hd); q_bound, k_bound, v_bound; q_rot,
    k_rot), or None if `mut` cannot show.  Rotated dims: rope_bound; the rest
    and V: 2^-8 |v| + 2^-16 A (the random family; the exact family compares
    bits)."""
    H = nh + nkv
    rows = d["s"].reshape(nh + 2 * nkv, hd)
    A = d["A"].reshape(nh + 2 * nkv, hd)
    if q_prior is None:                  # the op entry's sentinel fill
        q_prior = np.full((nh, hd), -STALE)
    r = rotate(rows, d["cos"], d["sin"], pos, nh, nkv, hd, rd, mut,
               q_prior=q_prior, k_prior=d["kc"][:, pos].astype(np.float64))
    if r is None:
        return None
    out, v, rot, a1, a2 = r
    half = rd // 2
    c = np.abs(np.asarray(d["cos"], np.float64)[pos])
    s = np.abs(np.asarray(d["sin"], np.float64)[pos])
    acc = np.zeros((H, hd))
    acc[:, :half] = A[:H, :half] * c + A[:H, half:rd] * s
    acc[:, half:rd] = A[:H, half:rd] * c + A[:H, :half] * s
    plain = lc.TOL_BF16 * np.abs(out) + lc.TOL_F32 * A[:H] + lc.ABS_EPS
    bound = np.where(rot, lc.rope_bound(np.abs(a1) + np.abs(a2), acc), plain)
    v_bound = lc.TOL_BF16 * np.abs(v) + lc.TOL_F32 * A[H:] + lc.ABS_EPS
    return dict(q=out[:nh], k=out[nh:], v=v, q_bound=bound[:nh],
                k_bound=bound[nh:], v_bound=v_bound, q_rot=rot[:nh],
                k_rot=rot[nh:])


def fused_sums_exact(d):
    """Exact family: every sum is exact in f32 however it is accumulated."""
    s = d["s"]
    return bool((s.astype(np.float32).astype(np.float64) == s).all() and
                (d["A"] < 2.0 ** 24).all())


def fused_moved(base, mutated, exact):
    for a in ("q", "k"):
        r = base[a + "_rot"]
        diff = np.abs(mutated[a] - base[a])
        if (diff[r] > 2 * base[a + "_bound"][r]).any():
            return True
        if exact:
            if (lr.bf16_bits(mutated[a][~r]) !=
                    lr.bf16_bits(base[a][~r])).any():
                return True
        elif (diff[~r] > 2 * base[a + "_bound"][~r]).any():
            return True
    if exact:
        return bool((lr.bf16_bits(mutated["v"]) !=
                     lr.bf16_bits(base["v"])).any())
    return bool((np.abs(mutated["v"] - base["v"]) >
                 2 * base["v_bound"]).any())
