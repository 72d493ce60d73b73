"""fp8 (e4m3) KV cache kernels against exact expectations (quantizer, scratch
fill) and a float64 reference over the dequantized cache (decode attention)."""
import functools
import math

import numpy as np
import pytest
import torch

import cake_amd
from tests.attn_cases import ABS_EPS, TOL_F32P, decode_max_seq, make_inputs
from tests.attn_ref import attn_ref
from tests.helpers import quantize_bf16

pytestmark = pytest.mark.gpu
NKV, MS = 2, 96


def e4m3(x):
    """Round-to-nearest-even e4m3 bytes of f32 x (torch's CPU conversion)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def e4m3_value(codes):
    t = torch.from_numpy(np.ascontiguousarray(codes)).view(torch.float8_e4m3fn)
    return t.to(torch.float32).numpy()


def row_k(row):
    amax = float(np.max(np.abs(row)))
    if amax == 0.0:
        return 0
    m, e = math.frexp(amax)  # 448 = 0.875 * 2^9
    return e - 9 if m <= 0.875 else e - 8


@pytest.mark.parametrize("pos0", [0, 45])
@pytest.mark.parametrize("S", [1, 5, 33])
def test_quant_rows_bit_exact(S, pos0):
    rng = np.random.default_rng(S * 100 + pos0)
    mag = 2.0 ** rng.integers(-9, 9, size=(2, NKV, MS, 1))
    x = quantize_bf16((rng.standard_normal((2, NKV, MS, 128)) * mag)
                      .astype(np.float32))
    # the four edge rows, all at pos0 so that S == 1 stores them too
    x[0, 0, pos0] = 0.0                                   # all-zero row
    x[0, 1, pos0] = np.clip(x[0, 1, pos0], -1.0, 1.0)
    x[0, 1, pos0, 5] = -448.0 * 8                         # amax = 448 * 2^3
    x[1, 0, pos0] = np.clip(x[1, 0, pos0], -1.0, 1.0)
    x[1, 0, pos0, 77] = 448.0 * 8 + 16                    # one bf16 step above
    small = 2.0 ** -10 * np.array([1, 2, 3, 4, 5, 6, 0.5, 16, -1, -3, -5, 64])
    x[1, 1, pos0] = np.resize(small, 128)                 # subnormal codes,
    x[1, 1, pos0, 3] = 256.0                              # ties, zeros; k = 0
    kc, vc = x[0], x[1]
    vtc = np.ascontiguousarray(vc.transpose(0, 2, 1))
    sent8 = np.full((NKV, MS, 128), 0x55, np.uint8)
    sents = np.full((NKV, MS), 123.0, np.float32)
    got = cake_amd.op_kv8_quant(kc, vc, vtc, sent8, sent8, sents, sents, pos0,
                                S, decode=(S == 1))
    gkc, gvc, gvtc, gk8, gv8, gks, gvs = got
    rows = slice(pos0, pos0 + S)
    for src, g16, g8, gs in ((kc, gkc, gk8, gks), (vc, gvc, gv8, gvs)):
        k = np.array([[row_k(r) for r in head] for head in src])
        scale = (2.0 ** k).astype(np.float32)
        codes = e4m3(src * (2.0 ** -k)[..., None].astype(np.float32))
        deq = e4m3_value(codes) * scale[..., None]
        assert np.array_equal(gs[:, rows], scale[:, rows])
        assert np.array_equal(g8[:, rows], codes[:, rows])
        assert np.array_equal(g16[:, rows], deq[:, rows])
        if src is vc:
            assert np.array_equal(gvtc[:, :, rows],
                                  deq.transpose(0, 2, 1)[:, :, rows])
        # everything outside the stored rows comes back as it went in
        out = np.ones(MS, bool)
        out[rows] = False
        assert np.array_equal(g16[:, out], src[:, out])
        assert np.all(g8[:, out] == 0x55) and np.all(gs[:, out] == 123.0)
    out = np.ones(MS, bool)
    out[rows] = False
    assert np.array_equal(gvtc[:, :, out], vtc[:, :, out])


@pytest.mark.parametrize("p0", [1, 64, 65])
@pytest.mark.parametrize("lo", [0, 7])
def test_dequant_rows_exact(lo, p0):
    rng = np.random.default_rng(lo * 100 + p0)
    valid = np.array([b for b in range(256) if b & 0x7F != 0x7F], np.uint8)
    k8 = rng.permutation(np.resize(valid, NKV * MS * 128)).reshape(NKV, MS, 128)
    v8 = rng.permutation(k8.reshape(-1)).reshape(NKV, MS, 128)
    assert len(np.unique(k8)) == 254
    ks = (2.0 ** rng.integers(-3, 4, size=(NKV, MS))).astype(np.float32)
    vs = (2.0 ** rng.integers(-3, 4, size=(NKV, MS))).astype(np.float32)
    sent = np.full((NKV, MS, 128), 7.0, np.float32)
    sent_t = np.full((NKV, 128, MS), 7.0, np.float32)
    gkc, gvc, gvtc = cake_amd.op_kv8_dequant(k8, v8, ks, vs, sent, sent,
                                             sent_t, lo, p0)
    ek = e4m3_value(k8) * ks[..., None]
    ev = e4m3_value(v8) * vs[..., None]
    inside = np.zeros(MS, bool)
    inside[lo:p0] = True
    ek[:, ~inside] = 7.0
    ev[:, ~inside] = 7.0
    assert np.array_equal(gkc, ek)
    assert np.array_equal(gvc, ev)
    assert np.array_equal(gvtc, ev.transpose(0, 2, 1))


# ---- decode attention -------------------------------------------------------
# Bound: the dequantized operands code * scale are exact in f32, so the error
# sources are those of the bf16 decode kernels with P kept in f32 (TOL_F32P =
# twice the derived 2^-8 * A worst case) plus two f32 multiplies per position
# (the K scale on the score, the V scale on the weight), 2 * 2^-24 relative:
# inside the factor-of-two margin.
GEOMS = [(4, 1), (2, 1), (1, 1), (8, 1), (8, 2), (7, 1), (3, 1)]
NS = [1, 2, 127, 128, 129, 300, 2100]


@functools.lru_cache(maxsize=4)
def decode_case(family, nh, nkv, n, window):
    """fp8 cache holding the family's content in [lo, n) under per-row scales
    2^-6..2^6, NaN codes and 2^60 scales everywhere else; float64 reference
    over code * scale."""
    ms = decode_max_seq(n)
    q, kc, vc = make_inputs(family, nh, nkv, 128, ms, 1, n - 1, window,
                            decode=True)
    rng = np.random.default_rng(n * 7 + window)
    lo = n - window if window and n > window else 0
    hidden = np.ones(ms, bool)
    hidden[lo:n] = False
    packed = []
    for x in (kc, vc):
        k = rng.integers(-6, 7, size=(nkv, ms))
        sc = (2.0 ** k).astype(np.float32)
        codes = e4m3(np.clip(x / sc[..., None], -448.0, 448.0))
        deq = e4m3_value(codes).astype(np.float64) * sc[..., None]
        codes[:, hidden] = 0x7F
        sc[:, hidden] = 2.0 ** 60
        deq[:, hidden] = 0.0
        packed += [codes, sc, deq]
    k8, ks, dk, v8, vs, dv = packed
    ref, A = attn_ref(q, dk, dv, n - 1, window)
    return q[0], k8, v8, ks, vs, ref[0], A[0]


@pytest.mark.parametrize("nchunk", [1, 4, 8])
@pytest.mark.parametrize("window", [0, 1, 65, 129])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("nh,nkv", GEOMS)
@pytest.mark.parametrize("family", ["peaky", "flat"])
def test_attn_decode_kv8_vs_float64(family, nh, nkv, n, window, nchunk):
    q, k8, v8, ks, vs, ref, A = decode_case(family, nh, nkv, n, window)
    # one case per geometry relaunches on one zeroing of cnt (modulo election)
    reps = 3 if (n, window) == (300, 0) and family == "peaky" else 1
    got = cake_amd.op_attn_decode_kv8(q, k8, v8, ks, vs, n - 1, window=window,
                                      nchunk=nchunk, repeats=reps)
    for r in range(reps):
        err = np.abs(got[r] - ref)
        bound = TOL_F32P * A + ABS_EPS
        worst = np.max(np.where(np.isnan(err), np.inf, err) / bound)
        print(f"launch {r}: max err / bound = {worst:.3f}")
        assert worst <= 1.0
