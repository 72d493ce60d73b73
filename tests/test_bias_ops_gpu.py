"""Op-level GPU parity (-m gpu) of the qwen2 q|k|v projection bias: the two
rope + KV-store kernels with a bias row, the biased fused decode kernel
k_gemv_qkv_rope_bias, and the existing GEMV / gate-up / 4-bit kernels at the
shapes the qwen2.5 configs reach.  Cases, inputs, references and bounds come
from tests/bias_cases.py; tests/test_bias_ref.py proves on the CPU that a
dropped, shifted, swapped or late-added bias exceeds twice what is granted
here.

Store kernels: every raw + b is exact in f32, so V, V^T and every untouched
slot (stale slots hold +-2^60) are bit-exact, q and K lie inside
kv_store_ref(raw + b)'s bound + 2^-24 (|x1| + |x2|).  Fused kernel: V bit-exact
in the exact family, q / k / random-family V inside the bounds of
bias_cases.fused_ref.  A NULL bias through either new entry equals the old
entry bit for bit.

Run with -s for the worst err / bound per kernel and the wall time per test
function (the table in DESIGN.md)."""
import collections
import time

import numpy as np
import pytest

import cake_amd
from tests import bias_cases as bc
from tests import linear_cases as lc
from tests import linear_ref as lr
from tests import w4_cases as wc
from tests import w4_ref as wr

pytestmark = pytest.mark.gpu
_id = lambda c: "-".join(map(str, c))

WORST = collections.defaultdict(float)
WALL = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nbias op tests: worst err/bound per kernel, wall per function")
    for k in sorted(WORST):
        print(f"  {k:36s} worst {WORST[k]:.3f}")
    for k in sorted(WALL):
        print(f"  wall {k:36s} {WALL[k]:6.2f} s")


@pytest.fixture(autouse=True)
def _wall(request):
    t = time.monotonic()
    yield
    WALL[request.node.originalname] += time.monotonic() - t


def _bits(a):
    return lr.f32_bits(a)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- store kernels ------------------------------------------------------------
@pytest.mark.parametrize("case", bc.store_cases(), ids=_id)
def test_kv_store_bias(case):
    nh, nkv, hd, S, pos0, decode = case
    kernel = "rope_store " + ("decode" if decode else "prefill") + " +bias"
    rows = slice(pos0, pos0 + S)
    other = np.ones(bc.STORE_MAX_SEQ, dtype=bool)
    other[rows] = False
    for fam in bc.STORE_FAMILIES:
        d = bc.store_inputs(fam, *case)
        r = bc.store_ref(d, nh, nkv, hd, pos0)
        gq, gk, gv, gvt = cake_amd.op_kv_store_bias(
            d["qkv"], d["bias"], d["cos"], d["sin"], d["kc"], d["vc"],
            d["vtc"], pos0, nh, nkv, eps=bc.EPS, decode=decode)
        eq = np.max(np.abs(gq - r["q"]) / r["qtol"])
        ek = np.max(np.abs(gk - r["kc"])[:, rows] / r["ktol"][:, rows])
        print(f"{kernel} {case} {fam}: q {eq:.3f} K {ek:.3f} of the bound")
        WORST[kernel] = max(WORST[kernel], eq, ek)
        assert eq <= 1.0, f"{fam}: q at {eq:.3f} of the bound"
        assert ek <= 1.0, f"{fam}: K at {ek:.3f} of the bound"
        # V = RNE_bf16(raw + b) bit for bit, V^T the same bits
        assert np.array_equal(lc.got_bits(gv[:, rows], False),
                              lr.bf16_bits(r["vc"][:, rows])), fam
        assert np.array_equal(_bits(gvt[:, :, rows]),
                              _bits(gv[:, rows].transpose(0, 2, 1))), fam
        # every other slot keeps its (stale) value
        assert np.array_equal(_bits(gk[:, other]), _bits(d["kc"][:, other]))
        assert np.array_equal(_bits(gv[:, other]), _bits(d["vc"][:, other]))
        assert np.array_equal(_bits(gvt[:, :, other]),
                              _bits(d["vtc"][:, :, other]))
    # NULL bias through the new entry == the old entry
    a = (d["qkv"], d["cos"], d["sin"], d["kc"], d["vc"], d["vtc"], pos0, nh,
         nkv)
    old = cake_amd.op_kv_store(*a, eps=bc.EPS, decode=decode)
    new = cake_amd.op_kv_store_bias(a[0], None, *a[1:], eps=bc.EPS,
                                    decode=decode)
    assert _same(old, new), "a NULL bias changed the store"


# ---- fused kernel -------------------------------------------------------------
@pytest.mark.parametrize("case", bc.fused_cases(), ids=_id)
def test_qkv_rope_bias(case):
    nh, nkv, hd, K, pos = case
    kb = cake_amd.linear_dispatch("qkv_rope", 128, K)["kb"]
    kernel = f"qkv_rope_bias KB{kb}"
    other = np.ones(lc.ROPE_MAX_SEQ, dtype=bool)
    other[pos] = False
    fails = []
    for fam in bc.FUSED_FAMILIES:
        d = bc.fused_inputs(fam, *case)
        r = bc.fused_ref(d, nh, nkv, hd, pos)
        q, rest, kc, vc, vtc = cake_amd.op_gemv_qkv_rope_bias(
            d["x"], d["nw"], d["w"], d["bias"], d["cos"], d["sin"], d["kc"],
            d["vc"], d["vtc"], pos, nh, nkv, eps=lc.EPS)
        if not np.array_equal(_bits(rest), _bits(np.full_like(
                rest, cake_amd.OP_SENTINEL))):
            fails.append(f"{fam}: the activation row past q was written")
        eq = np.max(np.abs(q - r["q"]) / r["q_bound"])
        ek = np.max(np.abs(kc[:, pos] - r["k"]) / r["k_bound"])
        WORST[kernel] = max(WORST[kernel], eq, ek)
        msg = f"{kernel} {case} {fam}: q {eq:.3f} k {ek:.3f}"
        if not (eq <= 1.0 and ek <= 1.0):
            fails.append(f"{fam}: q {eq:.3f}, k {ek:.3f} of the bound")
        if d["exact"]:
            if not np.array_equal(lc.got_bits(vc[:, pos], False),
                                  lr.bf16_bits(r["v"])):
                fails.append(f"{fam}: V differs from RNE_bf16(sum + b)")
        else:
            ev = np.max(np.abs(vc[:, pos] - r["v"]) / r["v_bound"])
            WORST[kernel] = max(WORST[kernel], ev)
            msg += f" v {ev:.3f}"
            if not ev <= 1.0:
                fails.append(f"{fam}: V at {ev:.3f} of the bound")
        print(msg + " of the bound")
        if not np.array_equal(_bits(vtc[:, :, pos]), _bits(vc[:, pos])):
            fails.append(f"{fam}: V^T column differs from the V row")
        for name, got, was in (("kc", kc[:, other], d["kc"][:, other]),
                               ("vc", vc[:, other], d["vc"][:, other]),
                               ("vtc", vtc[:, :, other],
                                d["vtc"][:, :, other])):
            if not np.array_equal(_bits(got), _bits(was)):
                fails.append(f"{fam}: {name} slot other than {pos} changed")
    # NULL bias through the new entry == the old entry (the unbiased kernel)
    a = (d["cos"], d["sin"], d["kc"], d["vc"], d["vtc"], pos, nh, nkv)
    old = cake_amd.op_gemv_qkv_rope(d["x"], d["nw"], d["w"], *a, eps=lc.EPS)
    new = cake_amd.op_gemv_qkv_rope_bias(d["x"], d["nw"], d["w"], None, *a,
                                         eps=lc.EPS)
    if not _same(old, new):
        fails.append("a NULL bias changed the fused kernel's output")
    assert not fails, "\n".join(fails)


def test_fused_equals_gemv_then_biased_store():
    """The two decode routes of a qwen2 layer (fused bf16; split GEMV + biased
    store, as fp8 / 4-bit / CAKE_BF16_SPLITNORM run) agree on V bit for bit in
    the exact family, where both add the same exact values."""
    nh, nkv, hd, K, pos = 14, 2, 64, 896, 45
    d = bc.fused_inputs("exact_dense", nh, nkv, hd, K, pos)
    _, _, kc, vc, vtc = cake_amd.op_gemv_qkv_rope_bias(
        d["x"], d["nw"], d["w"], d["bias"], d["cos"], d["sin"], d["kc"],
        d["vc"], d["vtc"], pos, nh, nkv, eps=lc.EPS)
    raw, _, _ = cake_amd.op_gemv(d["x"][None, :], d["w"], nw=d["nw"],
                                 eps=lc.EPS)
    _, k2, v2, vt2 = cake_amd.op_kv_store_bias(
        raw, d["bias"], d["cos"], d["sin"], d["kc"], d["vc"], d["vtc"], pos,
        nh, nkv, decode=True)
    assert np.array_equal(_bits(vc), _bits(v2))
    assert np.array_equal(_bits(vtc), _bits(vt2))


# ---- policy shapes the qwen2.5 configs reach (existing kernels) -----------------
N_POLICY = 64


@pytest.mark.parametrize("K", [896, 3584, 4864, 18944])
def test_gemv_at_qwen2_shapes(K):
    fam_k = cake_amd.linear_dispatch("plain", N_POLICY, K)
    assert fam_k["family"] == ("gemv_stream" if K > 16384 else "gemv_reg")
    for epi in (0, 1):
        for norm in (False, True) if K <= 16384 and epi == 0 else (False,):
            for fam in lc.gemv_families(norm):
                d = lc.gemv_inputs(fam, "bf16", N_POLICY, K, epi, norm)
                ref, A = lc.gemv_expect(d, epi, "fused" if norm else None)
                out, g, _ = cake_amd.op_gemv(
                    d["x"], d["w"], epi=epi, res=d["res"], alias=epi == 1,
                    nw=d["nw"] if norm else None, eps=lc.EPS)
                assert (g == cake_amd.OP_SENTINEL).all()
                if d["exact"]:
                    assert np.array_equal(lc.got_bits(out[0], False),
                                          lc.out_bits(ref, False)), (epi, fam)
                else:
                    err = np.max(np.abs(out[0] - ref) /
                                 (lc.gemv_tol(epi) * A + lc.ABS_EPS))
                    WORST[f"{fam_k['family']} K{K}"] = max(
                        WORST[f"{fam_k['family']} K{K}"], err)
                    assert err <= 1.0, (epi, norm, fam, err)


@pytest.mark.parametrize("K", [896, 3584])
def test_gateup_at_qwen2_shapes(K):
    for fam in lc.FAMILIES:
        d = lc.gateup_inputs(fam, False, N_POLICY, K, True)
        val, g, u, Ag, Au = lr.gateup_ref(d["W64"], d["x"], N_POLICY,
                                          d["nw"], lc.EPS)
        out, guards = cake_amd.op_gemv_gateup(d["x"], d["w"], N_POLICY,
                                              nw=d["nw"], eps=lc.EPS)
        assert (guards == cake_amd.OP_SENTINEL).all()
        err = np.max(np.abs(out - val) / lc.gateup_bound(val, g, u, Ag, Au))
        WORST[f"gateup K{K}"] = max(WORST[f"gateup K{K}"], err)
        assert err <= 1.0, (fam, err)


@pytest.mark.parametrize("K", [3584, 18944])
def test_gemv_w4_at_qwen2_shapes(K):
    g = 128
    for epi, alias in ((0, False), (1, True)):
        for fam in wc.FAMILIES:
            d = wc.gemv_inputs(fam, N_POLICY, K, g, epi, alias, 0, 1)
            out, guards = cake_amd.op_gemv_w4(d["x"], *d["t"], g, epi=epi,
                                              res=d["res"], rows=0,
                                              alias=alias)
            assert (guards == cake_amd.OP_SENTINEL).all()
            ref, A = wc.gemv_expect(d, g, 0)
            if d["exact"]:
                assert np.array_equal(wc.got_bits(out[0]),
                                      wr.bf16_bits(ref)), (epi, fam)
            else:
                err = np.max(np.abs(out[0] - ref) /
                             (wc.TOL_BF16 * A + wc.ABS_EPS))
                WORST[f"gemv_w4 K{K}"] = max(WORST[f"gemv_w4 K{K}"], err)
                assert err <= 1.0, (epi, fam, err)
