"""Float64 references for the attention kernels and the rope + KV-store step,
written from the definitions (independent of oracle.OracleModel and of
oracle.causal_mask; tests/test_attn_ref.py pins the two together).

Attention.  Query row i sits at absolute position p = pos0 + i and sees
    { j : j <= p and (window == 0 or j > p - window) };
head h reads kv-head h // (nh / nkv); scores are q.k / sqrt(hd); the softmax
is exact.  Besides out = P.V the reference returns A = P.|V|, the scale every
rounding error of a bf16 attention kernel is proportional to.

The two hooks exist for the CPU "teeth" tests only: they let a test compute
what a kernel with a wrong mask or a wrong head map WOULD produce."""
import numpy as np


def visible_set(S, pos0, window, n_slots):
    """(S, n_slots) bool, True where key slot j is visible to query row i."""
    p = pos0 + np.arange(S)[:, None]
    j = np.arange(n_slots)[None, :]
    vis = j <= p
    if window:
        vis = vis & (j > p - window)
    return vis


def attn_ref(q, kc, vc, pos0, window=0, vis_hook=None, kvmap_hook=None):
    """q (S, nh, hd); kc, vc (nkv, max_seq, hd).  Returns (out, A), both
    (S, nh*hd) float64.  vis_hook(vis, p) -> vis edits the visible set
    (p = (S, 1) absolute positions); kvmap_hook(h, kvh) -> kvh edits the
    head map."""
    q = np.asarray(q, dtype=np.float64)
    kc = np.asarray(kc, dtype=np.float64)
    vc = np.asarray(vc, dtype=np.float64)
    S, nh, hd = q.shape
    nkv, max_seq, _ = kc.shape
    assert nh % nkv == 0 and pos0 + S <= max_seq
    vis = visible_set(S, pos0, window, max_seq)
    if vis_hook is not None:
        vis = vis_hook(vis.copy(), pos0 + np.arange(S)[:, None])
    if not vis.any(axis=1).all():
        raise ValueError("a query row sees no key")
    out = np.empty((S, nh, hd))
    A = np.empty((S, nh, hd))
    for h in range(nh):
        kvh = h // (nh // nkv)
        if kvmap_hook is not None:
            kvh = kvmap_hook(h, kvh)
        s = (q[:, h, :] @ kc[kvh].T) / np.sqrt(float(hd))
        s = np.where(vis, s, -np.inf)
        e = np.exp(s - s.max(axis=1, keepdims=True))
        P = e / e.sum(axis=1, keepdims=True)
        out[:, h, :] = P @ vc[kvh]
        A[:, h, :] = P @ np.abs(vc[kvh])
    return out.reshape(S, nh * hd), A.reshape(S, nh * hd)


# ---- mutations of the reference (teeth tests) -----------------------------
# Each returns hook kwargs for attn_ref, or None when it does not apply to
# the shape (it would change nothing, or leave a row without any key).
def _vis_mut(edit):
    def make(S, pos0, window, max_seq, nh, nkv):
        base = visible_set(S, pos0, window, max_seq)
        p = pos0 + np.arange(S)[:, None]
        new = edit(base.copy(), p, window, max_seq)
        if new is None:
            return None
        # rows the edit would empty keep their true set
        empty = ~new.any(axis=1)
        new[empty] = base[empty]
        if np.array_equal(new, base):
            return None
        return dict(vis_hook=lambda vis, pp: new)
    return make


def _causal_plus1(vis, p, window, max_seq):
    rows = np.arange(vis.shape[0])
    ok = (p[:, 0] + 1) < max_seq
    vis[rows[ok], p[ok, 0] + 1] = True
    return vis


def _self_dropped(vis, p, window, max_seq):
    vis[np.arange(vis.shape[0]), p[:, 0]] = False
    return vis


def _window_delta(d):
    def edit(vis, p, window, max_seq):
        if window == 0 or window + d < 1:
            return None
        return visible_set(vis.shape[0], int(p[0, 0]), window + d, max_seq)
    return edit


def _oldest_dropped(vis, p, window, max_seq):
    first = vis.argmax(axis=1)
    vis[np.arange(vis.shape[0]), first] = False
    return vis


def _multiples_dropped(m):
    def edit(vis, p, window, max_seq):
        vis[:, ::m] = False
        return vis
    return edit


def _neighbour_kv(S, pos0, window, max_seq, nh, nkv):
    if nkv < 2:
        return None
    return dict(kvmap_hook=lambda h, kvh: (kvh + 1) % nkv)


MUTATIONS = {
    "causal+1": _vis_mut(_causal_plus1),
    "self_dropped": _vis_mut(_self_dropped),
    "window+1": _vis_mut(_window_delta(+1)),
    "window-1": _vis_mut(_window_delta(-1)),
    "oldest_dropped": _vis_mut(_oldest_dropped),
    "mult32_dropped": _vis_mut(_multiples_dropped(32)),
    "mult64_dropped": _vis_mut(_multiples_dropped(64)),
    "neighbour_kv_head": _neighbour_kv,
}


# ---- rope + KV store -------------------------------------------------------
def _bf16(a):
    """float64 -> nearest bf16 (RNE), returned as float64."""
    u = np.asarray(a, dtype=np.float64).astype(np.float32).view(np.uint32)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & np.uint32(0xFFFF0000)
    return r.view(np.float32).astype(np.float64)


def bf16_ulp(m):
    """Spacing of bf16 numbers at magnitude m (elementwise)."""
    m = np.abs(np.asarray(m, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(m, 2.0 ** -126)))
    return 2.0 ** (e - 7)


def kv_store_ref(qkv, cos, sin, pos0, nh, nkv, kc, vc, vtc, q_norm=None,
                 k_norm=None, eps=1e-6):
    """The store step on S raw rows (S, (nh+2*nkv)*hd) at positions pos0..:
    optional per-head QK-norm (x / sqrt(mean x^2 + eps) * w, re-quantized to
    bf16), HF half-rotation with the f32 cos/sin row of the position, K and V
    to slot p, V^T to column p.  Returns (q, kc, vc, vtc, qtol, ktol): the
    UNROUNDED float64 roped q (S, nh, hd) and new cache images (K unrounded),
    plus the element-wise bound for a correct bf16 kernel:
        one bf16 ulp of the result        (its single output rounding)
      + 2^-22 * (|x1| + |x2|)             (f32 arithmetic of the rotation)
      + with QK-norm only, one ulp of a normalized input times its |cos| or
        |sin| where that input lies within 2^-18 (relative) of a bf16
        rounding boundary: f32 and f64 may round it to different neighbours,
        and nothing but that is forgiven."""
    qkv = np.asarray(qkv, dtype=np.float64)
    S = qkv.shape[0]
    kc = np.array(kc, dtype=np.float64)
    vc = np.array(vc, dtype=np.float64)
    vtc = np.array(vtc, dtype=np.float64)
    hd = kc.shape[2]
    half = hd // 2
    rows = qkv.reshape(S, nh + 2 * nkv, hd)

    def rot(x, w, p):
        amb = np.zeros_like(x)
        if w is not None:
            sc = 1.0 / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + eps)
            y = x * sc * np.asarray(w, dtype=np.float64)
            x = _bf16(y)
            ulp = bf16_ulp(y)
            near_tie = np.abs(np.abs(y - x) - ulp / 2) < 2.0 ** -18 * np.abs(y)
            amb = np.where(near_tie, ulp, 0.0)
        c = np.asarray(cos[p], dtype=np.float64)
        s = np.asarray(sin[p], dtype=np.float64)
        x1, x2 = x[..., :half], x[..., half:]
        a1, a2 = amb[..., :half], amb[..., half:]
        mag = np.abs(x1) + np.abs(x2)
        out = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], axis=-1)
        slack = np.concatenate([a1 * np.abs(c) + a2 * np.abs(s),
                                a2 * np.abs(c) + a1 * np.abs(s)], axis=-1)
        return out, (bf16_ulp(out) + 2.0 ** -22 * np.concatenate([mag, mag],
                                                                 axis=-1)
                     + slack)

    q = np.empty((S, nh, hd))
    qtol = np.empty((S, nh, hd))
    ktol = np.zeros_like(kc)
    for i in range(S):
        p = pos0 + i
        q[i], qtol[i] = rot(rows[i, :nh], q_norm, p)
        kc[:, p, :], ktol[:, p, :] = rot(rows[i, nh:nh + nkv], k_norm, p)
        vc[:, p, :] = rows[i, nh + nkv:]
        vtc[:, :, p] = rows[i, nh + nkv:]
    return q, kc, vc, vtc, qtol, ktol
