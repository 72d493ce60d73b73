"""cake_amd — MI355X-native engine for cake's layer-sharded LLM hot path.

Host-side mirror of the reference's operator surface (ComputeBackend,
backends/mod.rs:40-685; Forwarder, cake/mod.rs:511-556; Topology YAML,
sharding/topology.rs) over the C-ABI of include/cake_hip.h.

The product path is the HIP engine in libcake_hip.so (hand-written gfx950
kernels + RCCL over xGMI).  There is NO CPU fallback: if the extension is
missing, importing this package raises, and every compute call requires a
real GPU.  The CPU oracle lives in oracle/ and is test infrastructure only.
"""
import ctypes
import json
import os

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_PKG_DIR, "libcake_hip.so")

COMM_ID_BYTES = 128
HAS_EMBED = 1
HAS_HEAD = 2
USE_GRAPH = 4
STATS = 8


class CakeHipError(RuntimeError):
    pass


def _load_lib():
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"cake_amd: native engine not built ({_LIB_PATH} missing). "
            "Run __graft_entry__.build() — there is no CPU fallback.")
    lib = ctypes.CDLL(_LIB_PATH)
    c = ctypes.c_int
    p = ctypes.c_void_p
    cp = ctypes.c_char_p
    fp = ctypes.POINTER(ctypes.c_float)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.cake_hip_last_error.restype = cp
    lib.cake_hip_build_info.restype = cp
    lib.cake_hip_engine_create.argtypes = [cp, c, c, c, c, c, c,
                                           ctypes.POINTER(p)]
    lib.cake_hip_engine_free.argtypes = [p]
    lib.cake_hip_topology_node_range.argtypes = [cp, cp, ctypes.POINTER(c),
                                                 ctypes.POINTER(c)]
    lib.cake_hip_load_safetensors.argtypes = [p, cp]
    lib.cake_hip_init_random.argtypes = [p, ctypes.c_uint64, ctypes.c_float]
    lib.cake_hip_prefill.argtypes = [p, u32p, c, u32p, fp]
    lib.cake_hip_decode.argtypes = [p, c, u32p]
    lib.cake_hip_reset.argtypes = [p]
    lib.cake_hip_forward_hidden.argtypes = [p, fp, c, c, fp]
    lib.cake_hip_forward_hidden_range.argtypes = [p, fp, c, c, c, c, fp]
    lib.cake_hip_comm_id.argtypes = [ctypes.c_char_p]
    lib.cake_hip_comm_init.argtypes = [p, c, c, ctypes.c_char_p]
    lib.cake_hip_op_rms_norm.argtypes = [c, c, ctypes.c_float, fp, fp, fp, c]
    lib.cake_hip_op_linear.argtypes = [c, c, c, fp, fp, fp, c]
    lib.cake_hip_op_silu_mul.argtypes = [ctypes.c_long, fp, fp, fp, c]
    lib.cake_hip_op_rope.argtypes = [c, c, c, c, fp, fp, fp, fp, c]
    f = ctypes.c_float
    lib.cake_hip_op_kv_store.argtypes = [c, c, c, c, c, c, c, fp, fp, fp, fp,
                                         fp, f, fp, fp, fp, fp, c]
    lib.cake_hip_op_kv_store_bias.argtypes = [c] * 7 + [fp] * 5 + [f] + \
        [fp] * 5 + [c]
    lib.cake_hip_op_kv_store_pr.argtypes = [c] * 8 + [fp] * 5 + [f] + \
        [fp] * 4 + [c]
    lib.cake_hip_op_attn_prefill.argtypes = [c] * 11 + [fp] * 5 + [c]
    lib.cake_hip_op_attn_decode.argtypes = [c] * 8 + [fp] * 4 + [c]
    lib.cake_hip_attn_dispatch.argtypes = [c, c, c, c, ctypes.POINTER(c)]
    lib.cake_hip_attn_decode_path.argtypes = [c, c, c, c]
    lib.cake_hip_attn_decode_group.argtypes = [c, c, c]
    lib.cake_hip_op_attn_decode_seq.argtypes = [c] * 7 + \
        [ctypes.POINTER(c)] + [fp] * 4 + [u32p, c]
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.cake_hip_op_gemv.argtypes = [c] * 7 + [fp, fp, u8p, fp, fp, fp, f, c,
                                               u32p, fp, fp, fp, c]
    lib.cake_hip_op_gemv_gateup.argtypes = [c, c, c, c, fp, fp, u8p, fp, fp,
                                            f, fp, fp, c]
    lib.cake_hip_op_gemv_qkv_rope.argtypes = [c] * 6 + [fp, fp, f] + \
        [fp] * 7 + [c]
    lib.cake_hip_op_gemv_qkv_rope_bias.argtypes = [c] * 6 + [fp, fp, f] + \
        [fp] * 8 + [c]
    lib.cake_hip_op_gemv_qkv_rope_pr.argtypes = [c] * 7 + [fp, fp, f] + \
        [fp] * 7 + [c]
    lib.cake_hip_op_gemm.argtypes = [c] * 6 + [fp, fp, fp, fp,
                                               ctypes.POINTER(c), c]
    lib.cake_hip_op_dequant_fp8.argtypes = [c, c, u8p, fp, fp, c]
    lib.cake_hip_op_silu_mul_rows.argtypes = [c, c, fp, fp, c]
    lib.cake_hip_op_rms_norm_rows.argtypes = [c, c, ctypes.c_long, c, f,
                                              ctypes.c_long, fp, fp, fp, c]
    lib.cake_hip_linear_dispatch.argtypes = [c, c, c, c, c,
                                             ctypes.POINTER(c)]
    lib.cake_hip_decode_dispatch.argtypes = [cp, ctypes.POINTER(c)]
    lib.cake_hip_rope_tables.argtypes = [cp, c, fp, fp, ctypes.POINTER(c)]
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.cake_hip_op_gemv_w4.argtypes = [c] * 7 + [fp, i32p, i32p, fp, fp, fp,
                                                  c]
    lib.cake_hip_op_gemv_gateup_w4.argtypes = [c] * 4 + [fp, i32p, i32p, fp,
                                                         fp, c]
    lib.cake_hip_op_dequant_w4.argtypes = [c] * 3 + [i32p, i32p, fp, fp, c]
    lib.cake_hip_linear_dispatch_w4.argtypes = [c, c, c, c,
                                                ctypes.POINTER(c)]
    lib.cake_hip_kernel_stats.argtypes = [p, ctypes.c_char_p, c]
    lib.cake_hip_stats_reset.argtypes = [p]
    lib.cake_hip_set_stats.argtypes = [p, c]
    lib.cake_hip_set_sampling.argtypes = [p, ctypes.c_float,
                                          ctypes.c_uint64]
    lib.cake_hip_set_sampling_ex.argtypes = [p, f, c, f, f, c,
                                             ctypes.c_uint64]
    lib.cake_hip_op_sample.argtypes = [c, fp, f, c, f, f, u32p, c,
                                       ctypes.c_uint64, c, c, u32p,
                                       ctypes.POINTER(c), fp, c]
    lib.cake_hip_op_argmax.argtypes = [c, fp, f, ctypes.c_uint64, c, c, c, c,
                                       u32p, fp, i32p, u32p,
                                       ctypes.POINTER(c), c]
    lib.cake_hip_op_embed.argtypes = [c, c, c, c, fp, u32p, f, fp, fp, c]
    lib.cake_hip_rope_tables_ex.argtypes = [cp, c, c, fp, fp,
                                            ctypes.POINTER(c)]
    lib.cake_hip_layer_dispatch.argtypes = [cp, c, ctypes.POINTER(c),
                                            ctypes.POINTER(c), fp]
    lib.cake_hip_op_postnorm_add.argtypes = [c, c, f, fp, fp, fp, fp, c]
    lib.cake_hip_op_gemv_gateup_gelu.argtypes = [c, c, c, fp, fp, fp, f, fp,
                                                 c]
    lib.cake_hip_op_gelu_mul_rows.argtypes = [c, c, fp, fp, c]
    lib.cake_hip_op_embed_scaled.argtypes = [c, c, c, c, fp, u32p, fp, c]
    lib.cake_hip_sync.argtypes = [p]
    return lib


_lib = _load_lib()


def _check(code):
    if code != 0:
        raise CakeHipError(_lib.cake_hip_last_error().decode())


def build_info():
    return _lib.cake_hip_build_info().decode()


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def topology_node_range(yaml_text: str, node: str):
    """Expand a cake topology YAML (topology.rs:134-169, incl. range
    expressions) to node's contiguous layer range [lo, hi)."""
    lo = ctypes.c_int()
    hi = ctypes.c_int()
    _check(_lib.cake_hip_topology_node_range(
        yaml_text.encode(), node.encode(), ctypes.byref(lo),
        ctypes.byref(hi)))
    return lo.value, hi.value


# ---------------------------------------------------------------------------
# op-level surface (kernel parity tests)
# ---------------------------------------------------------------------------
def op_rms_norm(x, w, eps=1e-5, device=0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows = int(np.prod(x.shape[:-1])) if x.ndim > 1 else 1
    cols = x.shape[-1]
    out = np.empty_like(x)
    _, xp = _f32(x)
    _, wp = _f32(w)
    _check(_lib.cake_hip_op_rms_norm(
        rows, cols, ctypes.c_float(eps), xp, wp,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out


def op_linear(x, w, device=0):
    """x (M,K) @ w(N,K)^T -> (M,N)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    M, K = x.shape
    N = w.shape[0]
    out = np.empty((M, N), dtype=np.float32)
    _, xp = _f32(x)
    _, wp = _f32(w)
    _check(_lib.cake_hip_op_linear(
        M, N, K, xp, wp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        device))
    return out


def op_silu_mul(gate, up, device=0):
    gate = np.ascontiguousarray(gate, dtype=np.float32)
    out = np.empty_like(gate)
    _, gp = _f32(gate)
    _, up_ = _f32(up)
    _check(_lib.cake_hip_op_silu_mul(
        gate.size, gp, up_,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out


def op_rope(x, cos, sin, device=0):
    """x (B,H,S,D), cos/sin (S, D/2)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b, h, s, d = x.shape
    out = np.empty_like(x)
    _, xp = _f32(x)
    _, cp = _f32(cos)
    _, sp = _f32(sin)
    _check(_lib.cake_hip_op_rope(
        b, h, s, d, xp, cp, sp,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out


def _f32_shaped(a, shape, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != tuple(shape):
        raise ValueError(f"{name}: shape {a.shape}, expected {tuple(shape)}")
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def op_kv_store(qkv, cos, sin, kc, vc, vtc, pos0, nh, nkv, q_norm=None,
                k_norm=None, eps=1e-6, decode=False, device=0):
    """Rope [+ QK-norm] + KV-cache store of raw qkv rows (S, (nh+2*nkv)*hd)
    at positions pos0.. (decode=True: the one-row decode kernel).  kc/vc
    (nkv, max_seq, hd) and vtc (nkv, hd, max_seq) are the PRIOR cache images;
    returns (roped q (S, nh, hd), kc, vc, vtc) after the store."""
    return _op_kv_store(False, None, qkv, cos, sin, kc, vc, vtc, pos0, nh,
                        nkv, q_norm, k_norm, eps, decode, device)


def op_kv_store_bias(qkv, bias, cos, sin, kc, vc, vtc, pos0, nh, nkv,
                     q_norm=None, k_norm=None, eps=1e-6, decode=False,
                     device=0):
    """op_kv_store through cake_hip_op_kv_store_bias: bias is the fused
    q|k|v projection bias row ((nh+2*nkv)*hd f32, qwen2), added to every raw
    row in f32 ahead of the rotation / the V store, or None."""
    return _op_kv_store(True, bias, qkv, cos, sin, kc, vc, vtc, pos0, nh, nkv,
                        q_norm, k_norm, eps, decode, device)


def op_kv_store_pr(qkv, cos, sin, kc, vc, vtc, pos0, nh, nkv, rd,
                   q_norm=None, k_norm=None, eps=1e-6, decode=False,
                   device=0):
    """op_kv_store through cake_hip_op_kv_store_pr: partial rotary, only the
    first rd dims of each q and k head rotate; cos / sin are (max_seq,
    rd/2)."""
    return _op_kv_store(False, None, qkv, cos, sin, kc, vc, vtc, pos0, nh,
                        nkv, q_norm, k_norm, eps, decode, device, rd=rd)


def _op_kv_store(bias_entry, bias, qkv, cos, sin, kc, vc, vtc, pos0, nh, nkv,
                 q_norm, k_norm, eps, decode, device, rd=None):
    kc = np.array(kc, dtype=np.float32, order="C")
    nkv_, max_seq, hd = kc.shape if kc.ndim == 3 else (0, 0, 0)
    half = (hd if rd is None else rd) // 2
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    S = qkv.shape[0]
    _, qp = _f32_shaped(qkv, (S, (nh + 2 * nkv) * hd), "qkv")
    kc, kp = _f32_shaped(kc, (nkv, max_seq, hd), "kc")
    vc, vp = _f32_shaped(np.array(vc, dtype=np.float32, order="C"),
                         (nkv, max_seq, hd), "vc")
    vtc, vtp = _f32_shaped(np.array(vtc, dtype=np.float32, order="C"),
                           (nkv, hd, max_seq), "vtc")
    _c, cp = _f32_shaped(cos, (max_seq, half), "cos")
    _s, sp = _f32_shaped(sin, (max_seq, half), "sin")
    qn = kn = qnp = knp = None
    if q_norm is not None:
        qn, qnp = _f32_shaped(q_norm, (hd,), "q_norm")
    if k_norm is not None:
        kn, knp = _f32_shaped(k_norm, (hd,), "k_norm")
    q_out = np.empty((S, nh, hd), dtype=np.float32)
    head = (S, pos0, 1 if decode else 0, nh, nkv, hd, max_seq, qp, cp, sp,
            qnp, knp, ctypes.c_float(eps))
    tail = (kp, vp, vtp,
            q_out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device)
    if rd is not None:
        _check(_lib.cake_hip_op_kv_store_pr(*head[:6], rd, *head[6:], *tail))
    elif bias_entry:
        _b, bp = _opt_f32(bias, ((nh + 2 * nkv) * hd,), "bias")
        _check(_lib.cake_hip_op_kv_store_bias(*head, bp, *tail))
    else:
        _check(_lib.cake_hip_op_kv_store(*head, *tail))
    return q_out, kc, vc, vtc


def op_attn_prefill(q, kc, vc, vtc, pos0, window=0, variant=None, device=0):
    """Prefill attention of post-rope q (S, nh, hd) at positions pos0.. over
    cache images kc/vc (nkv, max_seq, hd), vtc (nkv, hd, max_seq).  variant =
    (pfv, nw, split, deep); default: plain v2 NW=8 at hd 128, the MFMA-256
    kernel (1, 4, 0, 0) at hd 256 (its plain kernel is (0, 0, 0, 0)), else the
    generic kernel.  Returns (S, nh*hd)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    S, nh, hd = q.shape
    kc = np.ascontiguousarray(kc, dtype=np.float32)
    nkv, max_seq = kc.shape[0], kc.shape[1]
    if variant is None:
        variant = ((2, 8, 0, 0) if hd == 128 else
                   (1, 4, 0, 0) if hd == 256 else (0, 0, 0, 0))
    pfv, nw, split, deep = variant
    _, qp = _f32_shaped(q, (S, nh, hd), "q")
    _, kp = _f32_shaped(kc, (nkv, max_seq, hd), "kc")
    _v, vp = _f32_shaped(vc, (nkv, max_seq, hd), "vc")
    _t, vtp = _f32_shaped(vtc, (nkv, hd, max_seq), "vtc")
    out = np.empty((S, nh * hd), dtype=np.float32)
    _check(_lib.cake_hip_op_attn_prefill(
        S, pos0, nh, nkv, hd, max_seq, window, pfv, nw, split, deep, qp, kp,
        vp, vtp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out


def op_attn_decode(q, kc, vc, pos, window=0, nchunk=8, repeats=1, device=0):
    """Decode attention of q (nh, hd) at position pos over kc/vc (nkv,
    max_seq, hd); the kernel runs `repeats` times back to back on arrival
    counters zeroed once.  Returns (repeats, nh*hd)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    nh, hd = q.shape
    kc = np.ascontiguousarray(kc, dtype=np.float32)
    nkv, max_seq = kc.shape[0], kc.shape[1]
    _, qp = _f32_shaped(q, (nh, hd), "q")
    _, kp = _f32_shaped(kc, (nkv, max_seq, hd), "kc")
    _v, vp = _f32_shaped(vc, (nkv, max_seq, hd), "vc")
    out = np.empty((max(repeats, 0), nh * hd), dtype=np.float32)
    _check(_lib.cake_hip_op_attn_decode(
        nh, nkv, hd, max_seq, pos, window, nchunk, repeats, qp, kp, vp,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out


def op_sample(logits, temperature, top_k=0, top_p=1.0, repeat_penalty=1.0,
              history=(), seed=299792458, first_draw=0, draws=1, device=0):
    """The on-device sampler on f32 logits (V,): penalty over every id of
    `history`, top-k, top-p, then `draws` consecutive seeded draws from
    draw index first_draw.  Returns (tokens (draws,), kept, tau)."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    _, lp = _f32_shaped(logits, (logits.size,), "logits")
    hist = np.ascontiguousarray(history, dtype=np.uint32).reshape(-1)
    toks = np.empty(max(int(draws), 1), dtype=np.uint32)
    kept = ctypes.c_int()
    thr = ctypes.c_float()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _check(_lib.cake_hip_op_sample(
        logits.size, lp, temperature, int(top_k), top_p, repeat_penalty,
        hist.ctypes.data_as(u32p) if hist.size else None, hist.size, seed,
        int(first_draw), int(draws), toks.ctypes.data_as(u32p),
        ctypes.byref(kept), ctypes.byref(thr), device))
    return toks[:max(int(draws), 0)], kept.value, np.float32(thr.value)


def attn_dispatch(S, nh, nkv, hd):
    """The product's launch choices for this shape (host only): dict with the
    prefill variant and the grouped-decode grid_y (0 = per-head kernel)."""
    o = (ctypes.c_int * 6)()
    _check(_lib.cake_hip_attn_dispatch(S, nh, nkv, hd, o))
    return dict(pfv=o[0], nw=o[1], split=o[2], deep=o[3], split_min_s=o[4],
                decode_grid_y=o[5])


def attn_decode_path(nh, nkv, hd, nchunk):
    """The decode-attention kernel the product launches for this geometry and
    chunk count (host only): 0 per-head, 1 grouped, 2 short-context (the
    default at nchunk 4).  The library reads CAKE_ATTN_SHORT on every call:
    0 = never the short kernel, 2 = also at nchunk 8.  hd 256: 3."""
    return _lib.cake_hip_attn_decode_path(nh, nkv, hd, nchunk)


def attn_decode_group(nh, nkv, hd):
    """q-heads per block of the decode-attention kernel at this geometry
    (host only).  hd 256: the largest of 4, 3, 2, 1 dividing nh / nkv, capped
    by CAKE_ATTN256_GB, which the library reads on every call (default 1: the
    per-head route measured faster; 2..4 opt in to grouping)."""
    return _lib.cake_hip_attn_decode_group(nh, nkv, hd)


def op_attn_decode_seq(q, kc, vc, pos, nchunks, window=0, device=0):
    """op_attn_decode with a chunk count per launch, all launches back to
    back on one set of buffers.  Returns (out (len(nchunks), nh*hd), arrival
    counters (nh,) after the last launch; they start at 0)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    nh, hd = q.shape
    kc = np.ascontiguousarray(kc, dtype=np.float32)
    nkv, max_seq = kc.shape[0], kc.shape[1]
    _, qp = _f32_shaped(q, (nh, hd), "q")
    _, kp = _f32_shaped(kc, (nkv, max_seq, hd), "kc")
    _v, vp = _f32_shaped(vc, (nkv, max_seq, hd), "vc")
    nc = (ctypes.c_int * len(nchunks))(*[int(x) for x in nchunks])
    out = np.empty((len(nchunks), nh * hd), dtype=np.float32)
    cnt = np.empty(nh, dtype=np.uint32)
    _check(_lib.cake_hip_op_attn_decode_seq(
        nh, nkv, hd, max_seq, pos, window, len(nchunks), nc, qp, kp, vp,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), device))
    return out, cnt


# ---- linear-layer op entries (GEMV / fp8 / GEMM) --------------------------
OP_GUARD = 16                # guard elements behind every output buffer
OP_SENTINEL = -2.0 ** 60     # what outputs and guards are pre-filled with
GEMV_KINDS = {"bf16": 0, "fp8": 1, "splitk": 2}
GEMM_VARIANTS = {"128": 0, "256": 1, "128x256": 2, "256p": 3, "library": 4}
LINEAR_FAMILIES = ("gemv_reg", "gemv_stream", "gemv_fp8", "gemv_fp8_stream",
                   "gateup", "gateup_fp8", "qkv_rope", "splitk", "gemm",
                   "gemv_w4", "gateup_w4")
# families past the table above (CAKE_HIP_FAM_GATEUP_GELU = 11, gemma3)
GEMMA3_FAMILIES = ("gateup_gelu",)
LINEAR_KINDS = {"plain": 0, "gateup": 1, "qkv_rope": 2, "splitk": 3,
                "gemm": 4}


def _opt_f32(a, shape, name):
    if a is None:
        return None, None
    return _f32_shaped(a, shape, name)


def _u8(a, shape, name):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.shape != tuple(shape):
        raise ValueError(f"{name}: shape {a.shape}, expected {tuple(shape)}")
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def op_gemv(x, w, kind="bf16", sc=None, epi=0, res=None, nw=None, eps=1e-5,
            rows=0, alias=False, chain=0, cnt_init=None, scale_in=None,
            device=0):
    """One GEMV launcher (kind bf16 | fp8 | splitk) on x (repeats, K) [and
    res (repeats, N)], launched once per row back to back on counters set
    once from cnt_init.  w (N, K) is bf16-exact f32, or uint8 e4m3fn codes
    with sc (N/128, K/128).  chain 1 = norm-chain produce (cnt_init: 9
    words), 2 = consume (scale_in, nw).  Returns (out (repeats, N), guards
    (repeats, OP_GUARD), scale_out (repeats,) or None)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x = x[None] if x.ndim == 1 else x
    repeats, K = x.shape
    N = w.shape[0]
    k = GEMV_KINDS[kind]
    _, xp = _f32_shaped(x, (repeats, K), "x")
    wf = wfp = w8 = w8p = scp = None
    if k == 1:
        w8, w8p = _u8(w, (N, K), "w")
        _s, scp = _f32_shaped(sc, (N // 128, K // 128), "sc")
    else:
        wf, wfp = _f32_shaped(w, (N, K), "w")
    _r, rp = _opt_f32(res, (repeats, N), "res")
    _n, nwp = _opt_f32(nw, (K,), "nw")
    ci = cip = None
    if cnt_init is not None:
        ci = np.ascontiguousarray(
            np.broadcast_to(np.asarray(cnt_init, dtype=np.uint32), (9,)))
        cip = ci.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    si = sip = None
    if scale_in is not None:
        si, sip = _f32_shaped(np.float32(scale_in).reshape(1), (1,),
                              "scale_in")
    so = np.empty(repeats, dtype=np.float32) if chain == 1 else None
    out = np.empty((repeats, N + OP_GUARD), dtype=np.float32)
    fpp = ctypes.POINTER(ctypes.c_float)
    _check(_lib.cake_hip_op_gemv(
        k, N, K, epi, rows, 1 if alias else 0, repeats, xp, wfp, w8p, scp,
        rp, nwp, eps, chain, cip, sip,
        so.ctypes.data_as(fpp) if so is not None else None,
        out.ctypes.data_as(fpp), device))
    return out[:, :N], out[:, N:], so


def op_gemv_gateup(x, w, I, sc=None, nw=None, eps=1e-5, rows=0,
                   scale_in=None, device=0):
    """Fused [norm ->] gate-up GEMV -> silu_mul on x (K,), w (2I, K) bf16-
    exact f32 or uint8 fp8 codes with sc (2I/128, K/128).  Returns (out (I,),
    guards)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    K = x.shape[0]
    fp8 = sc is not None
    _, xp = _f32_shaped(x, (K,), "x")
    wfp = w8p = scp = None
    if fp8:
        _w, w8p = _u8(w, (2 * I, K), "w")
        _s, scp = _f32_shaped(sc, (2 * I // 128, K // 128), "sc")
    else:
        _w, wfp = _f32_shaped(w, (2 * I, K), "w")
    _n, nwp = _opt_f32(nw, (K,), "nw")
    si = sip = None
    if scale_in is not None:
        si, sip = _f32_shaped(np.float32(scale_in).reshape(1), (1,),
                              "scale_in")
    out = np.empty(I + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_gemv_gateup(
        1 if fp8 else 0, I, K, rows, xp, wfp, w8p, scp, nwp, eps, sip,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:I], out[I:]


def op_gemv_qkv_rope(x, nw, w, cos, sin, kc, vc, vtc, pos, nh, nkv,
                     eps=1e-5, device=0):
    """The fused norm -> qkv GEMV -> rope -> KV-store decode kernel.  kc/vc
    (nkv, max_seq, hd), vtc (nkv, hd, max_seq) are the PRIOR images.  Returns
    (roped q (nh, hd), rest of the activation row incl. guards, kc, vc,
    vtc)."""
    return _op_gemv_qkv_rope(False, None, x, nw, w, cos, sin, kc, vc, vtc,
                             pos, nh, nkv, eps, device)


def op_gemv_qkv_rope_bias(x, nw, w, bias, cos, sin, kc, vc, vtc, pos, nh, nkv,
                          eps=1e-5, device=0):
    """op_gemv_qkv_rope through cake_hip_op_gemv_qkv_rope_bias: bias is the
    fused q|k|v projection bias row ((nh+2*nkv)*hd f32), added to the f32
    sums ahead of the rotation / the V store (the biased kernel), or None (the
    unbiased one)."""
    return _op_gemv_qkv_rope(True, bias, x, nw, w, cos, sin, kc, vc, vtc, pos,
                             nh, nkv, eps, device)


def op_gemv_qkv_rope_pr(x, nw, w, cos, sin, kc, vc, vtc, pos, nh, nkv, rd,
                        eps=1e-5, device=0):
    """op_gemv_qkv_rope through cake_hip_op_gemv_qkv_rope_pr: partial rotary
    over the first rd dims of each head, cos / sin (max_seq, rd/2); rd < hd
    runs k_gemv_qkv_rope_pr, rd == hd the full-rotation kernel."""
    return _op_gemv_qkv_rope(False, None, x, nw, w, cos, sin, kc, vc, vtc,
                             pos, nh, nkv, eps, device, rd=rd)


def _op_gemv_qkv_rope(bias_entry, bias, x, nw, w, cos, sin, kc, vc, vtc, pos,
                      nh, nkv, eps, device, rd=None):
    kc = np.array(kc, dtype=np.float32, order="C")
    nkv_, max_seq, hd = kc.shape
    half = (hd if rd is None else rd) // 2
    x = np.ascontiguousarray(x, dtype=np.float32)
    K = x.shape[0]
    Nq = (nh + 2 * nkv) * hd
    _, xp = _f32_shaped(x, (K,), "x")
    _n, nwp = _f32_shaped(nw, (K,), "nw")
    _w, wp = _f32_shaped(w, (Nq, K), "w")
    _c, cp = _f32_shaped(cos, (max_seq, half), "cos")
    _s, sp = _f32_shaped(sin, (max_seq, half), "sin")
    kc, kp = _f32_shaped(kc, (nkv, max_seq, hd), "kc")
    vc, vp = _f32_shaped(np.array(vc, dtype=np.float32, order="C"),
                         (nkv, max_seq, hd), "vc")
    vtc, vtp = _f32_shaped(np.array(vtc, dtype=np.float32, order="C"),
                           (nkv, hd, max_seq), "vtc")
    out = np.empty(Nq + OP_GUARD, dtype=np.float32)
    head = (nh, nkv, hd, max_seq, pos, K, xp, nwp, eps, wp, cp, sp)
    tail = (kp, vp, vtp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            device)
    if rd is not None:
        _check(_lib.cake_hip_op_gemv_qkv_rope_pr(*head[:3], rd, *head[3:],
                                                 *tail))
    elif bias_entry:
        _b, bp = _opt_f32(bias, (Nq,), "bias")
        _check(_lib.cake_hip_op_gemv_qkv_rope_bias(*head, bp, *tail))
    else:
        _check(_lib.cake_hip_op_gemv_qkv_rope(*head, *tail))
    return out[:nh * hd].reshape(nh, hd), out[nh * hd:], kc, vc, vtc


def op_gemm(a, w, variant, res=None, alias=False, device=0):
    """a (M,K) @ w (N,K)^T [+ res (M,N)] by an explicit variant (a key of
    GEMM_VARIANTS).  Returns (out (M,N), guards, ran): ran is the variant
    name, or None when the library rejected the shape."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    M, K = a.shape
    N = w.shape[0]
    _, ap = _f32_shaped(a, (M, K), "a")
    _w, wp = _f32_shaped(w, (N, K), "w")
    _r, rp = _opt_f32(res, (M, N), "res")
    out = np.empty(M * N + OP_GUARD, dtype=np.float32)
    ran = ctypes.c_int(-2)
    _check(_lib.cake_hip_op_gemm(
        GEMM_VARIANTS[variant], M, N, K, 0 if res is None else 1,
        1 if alias else 0, ap, wp, rp,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        ctypes.byref(ran), device))
    name = None if ran.value < 0 else list(GEMM_VARIANTS)[ran.value]
    return out[:M * N].reshape(M, N), out[M * N:], name


def op_dequant_fp8(w8, sc, device=0):
    """Blockwise fp8 -> bf16 dequant of w8 (N,K) uint8 with sc (N/128,
    K/128).  Returns (out (N,K), guards)."""
    w8 = np.ascontiguousarray(w8, dtype=np.uint8)
    N, K = w8.shape
    _, wp = _u8(w8, (N, K), "w8")
    _s, scp = _f32_shaped(sc, (N // 128, K // 128), "sc")
    out = np.empty(N * K + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_dequant_fp8(
        N, K, wp, scp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        device))
    return out[:N * K].reshape(N, K), out[N * K:]


def op_silu_mul_rows(gu, device=0):
    """Prefill silu_mul on gu (S, 2I) = [gate | up].  Returns (out (S, I),
    guards)."""
    gu = np.ascontiguousarray(gu, dtype=np.float32)
    S, I = gu.shape[0], gu.shape[1] // 2
    _, gp = _f32_shaped(gu, (S, 2 * I), "gu")
    out = np.empty(S * I + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_silu_mul_rows(
        S, I, gp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:S * I].reshape(S, I), out[S * I:]


def op_rms_norm_rows(x, w, outer, inner, outer_stride, eps=1e-5, device=0):
    """rms_norm of outer*inner rows of len(w) elements inside the flat buffer
    x; row r starts at (r // inner) * outer_stride + (r % inner) * cols.
    Returns (out, same flat layout with sentinels between the rows,
    guards)."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(w, dtype=np.float32)
    _, xp = _f32_shaped(x, (x.size,), "x")
    _w, wp = _f32_shaped(w, (w.size,), "w")
    out = np.empty(x.size + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_rms_norm_rows(
        outer, inner, outer_stride, w.size, eps, x.size, xp, wp,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:x.size], out[x.size:]


# ---- head op entries (argmax / Gumbel draw, embedding gathers) -------------
ARGMAX_PARTS = 256                 # launch_argmax's partition count
OP_SENTINEL_BITS = 0xDD800000      # OP_SENTINEL as a 32-bit word
EMBED_MODES = {"rows": 0, "token": 1, "token_nscale": 2}


def op_argmax(logits, temperature=0.0, seed=299792458, first_step=0, steps=1,
              ring=True, advance_pos=1, device=0):
    """`steps` consecutive launch_argmax calls on f32 logits (V,), the device
    step counter starting at first_step and pos at 0.  ring=False passes a
    null ring.  Returns dict(tokens (steps,) the token word after each launch,
    pval (256,) f32 and pidx (256,) int32: the partials of the last launch,
    part_guards (2, OP_GUARD) uint32, ring (first_step + steps,) uint32 or
    None, ring_guards (OP_GUARD,) uint32 or None, pos, step).  Untouched
    words hold OP_SENTINEL_BITS."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    _, lp = _f32_shaped(logits, (logits.size,), "logits")
    n = max(int(steps), 1)
    G, NP = OP_GUARD, ARGMAX_PARTS
    toks = np.empty(n, dtype=np.uint32)
    pval = np.empty(NP + G, dtype=np.float32)
    pidx = np.empty(NP + G, dtype=np.int32)
    rbuf = np.empty(max(int(first_step), 0) + n + G, dtype=np.uint32)
    ps = (ctypes.c_int * 2)()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _check(_lib.cake_hip_op_argmax(
        logits.size, lp, temperature, seed, int(first_step), int(steps),
        1 if ring else 0, int(advance_pos), toks.ctypes.data_as(u32p),
        pval.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        pidx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
        rbuf.ctypes.data_as(u32p) if ring else None, ps, device))
    guards = np.stack([pval[NP:].view(np.uint32), pidx[NP:].view(np.uint32)])
    return dict(tokens=toks, pval=pval[:NP], pidx=pidx[:NP],
                part_guards=guards, ring=rbuf[:-G] if ring else None,
                ring_guards=rbuf[-G:] if ring else None, pos=ps[0],
                step=ps[1])


def op_embed(table, ids, mode="rows", eps=1e-5, device=0):
    """The embedding gathers on table (Vt, H) (f32, uploaded through the
    f32 -> bf16 conversion).  mode "rows": launch_embed_rows on ids (S,);
    "token": launch_embed_token on one id; "token_nscale": the same with the
    fp8 norm chain's nscale.  Returns (out (S, H) f32, guards (OP_GUARD,),
    nscale f32 (OP_SENTINEL unless requested), nscale guards (OP_GUARD,))."""
    table = np.ascontiguousarray(table, dtype=np.float32)
    if table.ndim != 2:
        raise ValueError(f"table: shape {table.shape}, expected (Vt, H)")
    Vt, H = table.shape
    _, tp = _f32_shaped(table, (Vt, H), "table")
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    S = ids.size
    out = np.empty(S * H + OP_GUARD, dtype=np.float32)
    ns = np.empty(1 + OP_GUARD, dtype=np.float32)
    fpp = ctypes.POINTER(ctypes.c_float)
    _check(_lib.cake_hip_op_embed(
        Vt, H, S, EMBED_MODES[mode], tp,
        ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), eps,
        out.ctypes.data_as(fpp), ns.ctypes.data_as(fpp), device))
    return out[:S * H].reshape(S, H), out[S * H:], ns[0], ns[1:]


def linear_dispatch(kind, n, K, M=1, fp8=False):
    """The product's kernel choice for a linear layer (host only).  kind is a
    key of LINEAR_KINDS; n = N (or I for gateup).  Returns dict(family, rows,
    kb (0 = streaming kernel), lib_first, variant)."""
    o = (ctypes.c_int * 5)()
    _check(_lib.cake_hip_linear_dispatch(LINEAR_KINDS[kind], n, K, M,
                                         1 if fp8 else 0, o))
    d = dict(family=LINEAR_FAMILIES[o[0]], rows=o[1], kb=o[2])
    if kind == "gemm":
        d = dict(family="gemm", lib_first=bool(o[3]),
                 variant=list(GEMM_VARIANTS)[o[4]])
    return d


# ---- GPTQ 4-bit op entries (checkpoint-layout tensors) ---------------------
def _i32(a, shape, name):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.shape != tuple(shape):
        raise ValueError(f"{name}: shape {a.shape}, expected {tuple(shape)}")
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _w4_tensors(qweight, qzeros, scales, group):
    """(N, K, g, pointers) of one gptq projection in checkpoint layout:
    qweight (K/8, N) int32, qzeros (K/g, N/8) int32, scales (K/g, N)."""
    qweight = np.asarray(qweight)
    K, N = qweight.shape[0] * 8, qweight.shape[1]
    g = K if group == -1 else int(group)
    G = K // g if g > 0 else 0
    qw = _i32(qweight, (K // 8, N), "qweight")
    qz = _i32(qzeros, (G, N // 8), "qzeros")
    sc = _f32_shaped(scales, (G, N), "scales")
    return N, K, g, qw, qz, sc


def op_gemv_w4(x, qweight, qzeros, scales, group, epi=0, res=None, rows=0,
               alias=False, device=0):
    """The 4-bit GEMV on x (repeats, K) [and res (repeats, N)], one launch per
    row back to back.  Returns (out (repeats, N), guards (repeats,
    OP_GUARD))."""
    N, K, g, qw, qz, sc = _w4_tensors(qweight, qzeros, scales, group)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x = x[None] if x.ndim == 1 else x
    repeats = x.shape[0]
    _, xp = _f32_shaped(x, (repeats, K), "x")
    _r, rp = _opt_f32(res, (repeats, N), "res")
    out = np.empty((repeats, N + OP_GUARD), dtype=np.float32)
    _check(_lib.cake_hip_op_gemv_w4(
        N, K, g, epi, rows, 1 if alias else 0, repeats, xp, qw[1], qz[1],
        sc[1], rp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        device))
    return out[:, :N], out[:, N:]


def op_gemv_gateup_w4(x, qweight, qzeros, scales, group, rows=0, device=0):
    """The 4-bit gate-up GEMV -> silu_mul on normalized x (K,); the tensors
    hold N = 2I columns, gate then up.  Returns (out (I,), guards)."""
    N, K, g, qw, qz, sc = _w4_tensors(qweight, qzeros, scales, group)
    I = N // 2
    _, xp = _f32_shaped(np.ascontiguousarray(x, dtype=np.float32), (K,), "x")
    out = np.empty(I + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_gemv_gateup_w4(
        I, K, g, rows, xp, qw[1], qz[1], sc[1],
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:I], out[I:]


def op_dequant_w4(qweight, qzeros, scales, group, device=0):
    """4-bit -> bf16 dequant of one projection.  Returns (out (N, K),
    guards)."""
    N, K, g, qw, qz, sc = _w4_tensors(qweight, qzeros, scales, group)
    out = np.empty(N * K + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_dequant_w4(
        N, K, g, qw[1], qz[1], sc[1],
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:N * K].reshape(N, K), out[N * K:]


def linear_dispatch_w4(kind, n, K, group=128):
    """The 4-bit kernel choice (host only) for kind "plain" (n = N) or
    "gateup" (n = I).  Returns dict(family, rows, kb)."""
    o = (ctypes.c_int * 5)()
    _check(_lib.cake_hip_linear_dispatch_w4(LINEAR_KINDS[kind], n, K, group,
                                            o))
    return dict(family=LINEAR_FAMILIES[o[0]], rows=o[1], kb=o[2])


def decode_dispatch(config):
    """The five linear launches of one decode step of a model (host only), by
    the engine's own predicates: {layer: (family, rows, kb)} for qkv, o,
    gateup, down, head."""
    if isinstance(config, dict):
        config = json.dumps(config)
    o = (ctypes.c_int * 15)()
    _check(_lib.cake_hip_decode_dispatch(config.encode(), o))
    fams = LINEAR_FAMILIES + GEMMA3_FAMILIES
    return {k: (fams[o[3 * i]], o[3 * i + 1], o[3 * i + 2])
            for i, k in enumerate(("qkv", "o", "gateup", "down", "head"))}


def rope_tables(config, max_seq, local=False):
    """The rope tables engine create builds for this config and max_seq (host
    only, same function): (cos, sin), each (max_seq, rd/2) f32, rd the rotated
    dims of a head (partial_rotary_factor); LongRoPE's list choice and
    attention factor included.  local=True: the table of a gemma3 config's
    local (sliding) layers; the default is its global layers' table."""
    if isinstance(config, dict):
        config = json.dumps(config)
    rd = ctypes.c_int(0)
    which = 1 if local else 0
    _check(_lib.cake_hip_rope_tables_ex(config.encode(), max_seq, which, None,
                                        None, ctypes.byref(rd)))
    cos = np.empty((max_seq, rd.value // 2), dtype=np.float32)
    sin = np.empty_like(cos)
    fpt = ctypes.POINTER(ctypes.c_float)
    _check(_lib.cake_hip_rope_tables_ex(config.encode(), max_seq, which,
                                        cos.ctypes.data_as(fpt),
                                        sin.ctypes.data_as(fpt),
                                        ctypes.byref(rd)))
    return cos, sin


def layer_dispatch(config, layer):
    """What engine create plans for one layer of a model (host only):
    dict(window (0 = full attention), rope_table ("global" | "local": which
    of a gemma3 config's two tables), q_scale (the factor folded into the
    q-norm row: sqrt(head_dim / query_pre_attn_scalar) for gemma3, else 1))."""
    if isinstance(config, dict):
        config = json.dumps(config)
    win, tab, qs = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    _check(_lib.cake_hip_layer_dispatch(config.encode(), int(layer),
                                        ctypes.byref(win), ctypes.byref(tab),
                                        ctypes.byref(qs)))
    return dict(window=win.value, rope_table=("global", "local")[tab.value],
                q_scale=np.float32(qs.value))


# ---- gemma3 op entries ------------------------------------------------------
def op_postnorm_add(x, t, w, eps=1e-6, device=0):
    """x (S, H) + rms_norm(t) * w with HF's bf16 rounding points (the normed
    value, then the sum); S == 1 runs the decode launch.  Returns (out (S, H),
    guards)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    S, H = x.shape
    _, xp = _f32_shaped(x, (S, H), "x")
    _t, tp = _f32_shaped(t, (S, H), "t")
    _w, wp = _f32_shaped(w, (H,), "w")
    out = np.empty(S * H + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_postnorm_add(
        S, H, eps, xp, tp, wp,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:S * H].reshape(S, H), out[S * H:]


def op_gemv_gateup_gelu(x, w, I, nw=None, eps=1e-6, rows=0, device=0):
    """op_gemv_gateup's bf16 form with the GELU-tanh gate.  Returns (out (I,),
    guards)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    K = x.shape[0]
    _, xp = _f32_shaped(x, (K,), "x")
    _w, wp = _f32_shaped(w, (2 * I, K), "w")
    _n, nwp = _opt_f32(nw, (K,), "nw")
    out = np.empty(I + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_gemv_gateup_gelu(
        I, K, rows, xp, wp, nwp, eps,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:I], out[I:]


def op_gelu_mul_rows(gu, device=0):
    """Prefill gelu_mul on gu (S, 2I) = [gate | up].  Returns (out (S, I),
    guards)."""
    gu = np.ascontiguousarray(gu, dtype=np.float32)
    S, I = gu.shape[0], gu.shape[1] // 2
    _, gp = _f32_shaped(gu, (S, 2 * I), "gu")
    out = np.empty(S * I + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_gelu_mul_rows(
        S, I, gp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:S * I].reshape(S, I), out[S * I:]


def op_embed_scaled(table, ids, mode="rows", device=0):
    """The gemma3 embedding gathers (rows times bf16(sqrt(H)), rounded to
    bf16) on table (Vt, H); mode "rows" or "token".  Returns (out (S, H),
    guards)."""
    table = np.ascontiguousarray(table, dtype=np.float32)
    if table.ndim != 2:
        raise ValueError(f"table: shape {table.shape}, expected (Vt, H)")
    Vt, H = table.shape
    _, tp = _f32_shaped(table, (Vt, H), "table")
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    S = ids.size
    out = np.empty(S * H + OP_GUARD, dtype=np.float32)
    _check(_lib.cake_hip_op_embed_scaled(
        Vt, H, S, {"rows": 0, "token": 1}[mode], tp,
        ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), device))
    return out[:S * H].reshape(S, H), out[S * H:]


def comm_id() -> bytes:
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(_lib.cake_hip_comm_id(buf))
    return buf.raw


# ---------------------------------------------------------------------------
# Engine — host mirror of Master/TextModelBase over the C-ABI
# ---------------------------------------------------------------------------
class Engine:
    def __init__(self, config, layer_lo=0, layer_hi=None, flags=None,
                 max_seq=0, max_batch_tokens=0, device=0):
        if isinstance(config, dict):
            config = json.dumps(config)
        cfg = json.loads(config)
        if cfg.get("model_type") == "gemma3":
            # the multimodal form: the text model's fields, HF's defaults
            # for what it leaves out
            cfg = {"num_hidden_layers": 26, "vocab_size": 262208,
                   "hidden_size": 2304, **(cfg.get("text_config") or {})}
        if layer_hi is None:
            layer_hi = cfg["num_hidden_layers"]
        if flags is None:
            flags = HAS_EMBED | HAS_HEAD | USE_GRAPH
        self.cfg = cfg
        self.flags = flags
        self.vocab = cfg.get("vocab_size", 0)
        self.hidden = cfg.get("hidden_size", 0)
        h = ctypes.c_void_p()
        _check(_lib.cake_hip_engine_create(
            config.encode(), layer_lo, layer_hi, flags, max_seq,
            max_batch_tokens, device, ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_topology(cls, config, topology_yaml, node, **kw):
        lo, hi = topology_node_range(topology_yaml, node)
        return cls(config, layer_lo=lo, layer_hi=hi, **kw)

    def load_safetensors(self, path):
        _check(_lib.cake_hip_load_safetensors(self._h, path.encode()))

    def init_random(self, seed=299792458, scale=0.02):
        _check(_lib.cake_hip_init_random(self._h, seed, ctypes.c_float(scale)))

    def comm_init(self, rank, world, comm_id_bytes):
        _check(_lib.cake_hip_comm_init(self._h, rank, world, comm_id_bytes))

    def prefill(self, tokens, want_logits=False):
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        nxt = ctypes.c_uint32()
        logits = np.empty(self.vocab, dtype=np.float32) if want_logits else None
        _check(_lib.cake_hip_prefill(
            self._h,
            tokens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            len(tokens), ctypes.byref(nxt),
            logits.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            if want_logits else None))
        return (nxt.value, logits) if want_logits else nxt.value

    def prefill_participate(self, n_tokens):
        """Non-rank-0 side of a pipelined prefill."""
        _check(_lib.cake_hip_prefill(self._h, None, n_tokens, None, None))

    def decode(self, steps):
        out = np.empty(steps, dtype=np.uint32)
        _check(_lib.cake_hip_decode(
            self._h, steps,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def decode_participate(self, steps):
        _check(_lib.cake_hip_decode(self._h, steps, None))

    def forward_hidden(self, x, index_pos=0):
        """Run this shard's blocks on (seq, hidden) f32 hidden states —
        the Forwarder::forward_batch unit (cake/mod.rs:533-540)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        seq = x.shape[0]
        out = np.empty_like(x)
        _check(_lib.cake_hip_forward_hidden(
            self._h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), seq,
            index_pos, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out

    def forward_hidden_range(self, x, index_pos, layer_lo, layer_hi):
        """forward_hidden over the contiguous sub-range [layer_lo, layer_hi)
        of this shard's layers (absolute indices) — the per-op unit of the
        reference worker loop (worker.rs:442-515)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        seq = x.shape[0]
        out = np.empty_like(x)
        _check(_lib.cake_hip_forward_hidden_range(
            self._h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), seq,
            index_pos, layer_lo, layer_hi,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out

    def reset(self):
        _check(_lib.cake_hip_reset(self._h))

    def sync(self):
        _check(_lib.cake_hip_sync(self._h))

    def set_sampling(self, temperature, seed=299792458):
        """temperature <= 0 = greedy ArgMax (cake's convention,
        text_model.rs:104); > 0 = on-GPU Gumbel-argmax sampling."""
        _check(_lib.cake_hip_set_sampling(
            self._h, ctypes.c_float(temperature), seed))

    def set_sampling_ex(self, temperature, top_k=0, top_p=1.0,
                        repeat_penalty=1.0, repeat_last_n=128,
                        seed=299792458):
        """set_sampling plus on-GPU top-k, top-p and cake's repeat penalty
        (text_model.rs:433-452) inside the decode graph; semantics in
        include/cake_hip.h.  All three off == set_sampling."""
        _check(_lib.cake_hip_set_sampling_ex(
            self._h, temperature, int(top_k or 0),
            1.0 if top_p is None else top_p, repeat_penalty,
            int(repeat_last_n), seed))

    def set_stats(self, enabled):
        _check(_lib.cake_hip_set_stats(self._h, 1 if enabled else 0))

    def stats_reset(self):
        _check(_lib.cake_hip_stats_reset(self._h))

    def kernel_stats(self):
        buf = ctypes.create_string_buffer(1 << 20)
        _check(_lib.cake_hip_kernel_stats(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def generate_greedy(self, prompt_ids, max_new):
        """Greedy generation mirroring Master::generate_text's loop
        (master.rs:109-171): prefill produces token 0, decode the rest."""
        self.reset()
        first = self.prefill(prompt_ids)
        if max_new == 1:
            return [first]
        rest = self.decode(max_new - 1)
        return [first] + list(rest)

    def close(self):
        if self._h:
            _lib.cake_hip_engine_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
