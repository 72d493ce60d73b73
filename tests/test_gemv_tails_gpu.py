"""The decode GEMV kernels whose loads were moved ahead of their consumers
(residual row of k_gemv_reg EPI 1, pos + cos/sin of k_gemv_qkv_rope, the
first weight slab of k_gemv_gateup with the fused norm) against the float64
references of tests/linear_ref.py, at the smallest shapes that reach each
changed path (-m gpu).  Inputs, references and bounds are those of
test_linear_ops_gpu.py."""
import numpy as np
import pytest

import cake_amd
from tests import linear_cases as lc
from tests import linear_ref as lr

pytestmark = pytest.mark.gpu


def _guards(tag, g, fails):
    if not np.array_equal(lr.f32_bits(g),
                          lr.f32_bits(np.full_like(g, cake_amd.OP_SENTINEL))):
        fails.append(f"{tag}: a guard element past the output was written")


def _judge(tag, exact, got, ref, bound, fails):
    got = np.asarray(got, dtype=np.float32)
    if exact:
        bad = lc.got_bits(got, False) != lc.out_bits(ref, False)
        if bad.any():
            fails.append(f"{tag}: {bad.sum()} of {bad.size} elements differ "
                         "from the exact result")
        return
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    worst = np.inf if np.isnan(got).any() else float(np.max(ratio))
    if not worst <= 1.0:
        fails.append(f"{tag}: err/bound = {worst:.3f}")


@pytest.mark.parametrize("rows", lc.GEMV_ROWS)
@pytest.mark.parametrize("K", [4096, 14336])
def test_gemv_residual_in_place(K, rows):
    """EPI 1 with res aliasing out, N = 2 * rows + 1: the last block is
    ragged, so the clamped residual prefetch is exercised; three launches
    with different x and residual rows."""
    N = lc.gemv_n(rows)
    fails = []
    for norm in (None, "fused"):
        for fam in lc.gemv_families(norm is not None):
            d = lc.gemv_inputs(fam, "bf16", N, K, 1, norm is not None,
                               repeats=3)
            kw = dict(kind="bf16", epi=1, res=d["res"], rows=rows, alias=True,
                      eps=lc.EPS)
            if norm:
                kw["nw"] = d["nw"]
            out, g, _ = cake_amd.op_gemv(d["x"], d["w"], **kw)
            _guards(f"{norm}/{fam}", g, fails)
            for i in range(3):
                ref, A = lc.gemv_expect(d, 1, norm, i)
                _judge(f"{norm}/{fam}/repeat{i}", d["exact"], out[i], ref,
                       lc.gemv_tol(1) * A + lc.ABS_EPS, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("K", [72, 4104])
@pytest.mark.parametrize("pos", lc.ROPE_POS)
def test_qkv_rope_positions(K, pos):
    """pos 0, a middle position and max_seq - 1 on the smallest geometry the
    fused kernel takes (KB 1 and the product's KB 2)."""
    nh, nkv, hd = lc.ROPE_GEOM[0]
    fails = []
    for fam in ("exact_dense", "random"):
        d = lc.rope_inputs(fam, nh, nkv, hd, K, pos)
        r = lr.qkv_rope_ref(d["w"], d["x"], d["nw"], lc.EPS, d["cos"],
                            d["sin"], pos, nh, nkv, hd, d["kc"], d["vc"],
                            d["vtc"])
        q, rest, kc, vc, vtc = cake_amd.op_gemv_qkv_rope(
            d["x"], d["nw"], d["w"], d["cos"], d["sin"], d["kc"], d["vc"],
            d["vtc"], pos, nh, nkv, eps=lc.EPS)
        _guards(f"{fam}/activation row", rest, fails)
        _judge(f"{fam}/q", False, q, r["q"],
               lc.rope_bound(r["q_mag"], r["q_acc"]), fails)
        _judge(f"{fam}/k", False, kc[:, pos], r["kc"][:, pos],
               lc.rope_bound(r["k_mag"], r["k_acc"]), fails)
        if d["exact"]:
            if not np.array_equal(lc.got_bits(vc[:, pos], False),
                                  lr.bf16_bits(r["vc"][:, pos])):
                fails.append(f"{fam}: V row differs from bf16 of the sum")
        else:
            s = r["vc"][:, pos]
            _judge(f"{fam}/v", False, vc[:, pos], s,
                   lc.TOL_BF16 * np.abs(s) + lc.TOL_F32 * r["v_A"] +
                   lc.ABS_EPS, fails)
        if not np.array_equal(lr.f32_bits(vtc[:, :, pos]),
                              lr.f32_bits(vc[:, pos])):
            fails.append(f"{fam}: V^T column differs from the V row")
        other = np.ones(lc.ROPE_MAX_SEQ, dtype=bool)
        other[pos] = False
        for name, got, was in (("kc", kc[:, other], d["kc"][:, other]),
                               ("vc", vc[:, other], d["vc"][:, other]),
                               ("vtc", vtc[:, :, other],
                                d["vtc"][:, :, other])):
            if not np.array_equal(lr.f32_bits(got), lr.f32_bits(was)):
                fails.append(f"{fam}: {name} slot other than {pos} changed")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rows", [4, 8])
def test_gateup_fused_norm_k4096(rows):
    """KB 2 with the fused norm: the first weight slab is requested ahead of
    the norm's barriers.  I = 2 * rows + 1 leaves a ragged last block."""
    K, I = 4096, lc.gateup_i(False, rows)
    fails = []
    for fam in lc.gemv_families(True):
        d = lc.gateup_inputs(fam, False, I, K, True)
        val, g, u, Ag, Au = lr.gateup_ref(d["W64"], d["x"], I, d["nw"],
                                          lc.EPS, None, None, False)
        out, gd = cake_amd.op_gemv_gateup(d["x"], d["w"], I, sc=d["sc"],
                                          eps=lc.EPS, rows=rows, nw=d["nw"])
        _guards(fam, gd, fails)
        _judge(fam, False, out, val, lc.gateup_bound(val, g, u, Ag, Au),
               fails)
    assert not fails, "\n".join(fails)
