"""Op-level GPU parity (-m gpu) of partial rotary (rd < hd): the two rope +
KV-store kernels called with the real rd, and the partial-rotary fused decode
kernel k_gemv_qkv_rope_pr.  Cases, inputs, references and bounds come from
tests/rotary_cases.py; tests/test_rotary_ref.py proves on the CPU that a wrong
pairing, a rotated, unwritten, shifted or neighbouring pass-through block, a
table stride of hd/2 or a V column offset exceeds twice what is granted here.

Store kernels: the raw rows are bf16, so q's and K's pass-through dims, V, V^T
and every untouched slot (stale slots hold +-2^60) are bit-exact; rotated dims
lie inside kv_store_ref's bound.  Fused kernel: pass-through dims and V are
bit-exact in the exact family; rotated dims, and the random family's other
dims, lie inside the bounds of rotary_cases.fused_ref.  rd == hd through either
new entry equals the old entry bit for bit, and so do three repeats.

Run with -s for the worst err / bound per kernel and the wall time per test
function (the table in DESIGN.md)."""
import collections
import itertools
import time

import numpy as np
import pytest

import cake_amd
from tests import linear_cases as lc
from tests import linear_ref as lr
from tests import rotary_cases as rc

pytestmark = pytest.mark.gpu
_id = lambda c: "-".join(map(str, c))

WORST = collections.defaultdict(float)
WALL = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nrotary op tests: worst err/bound per kernel, wall per function")
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


def _groups(cases, key):
    return [list(g) for _, g in itertools.groupby(cases, key=key)]


# ---- store kernels ------------------------------------------------------------
@pytest.mark.parametrize("cases", _groups(rc.store_cases(), lambda c: c[:4]),
                         ids=lambda g: _id(g[0][:4]))
def test_kv_store_pr(cases):
    fails = []
    for case in cases:
        nh, nkv, hd, rd, S, pos0, decode = case
        kernel = "rope_store " + ("decode" if decode else "prefill") + " rd<hd"
        rows = slice(pos0, pos0 + S)
        other = np.ones(rc.STORE_MAX_SEQ, dtype=bool)
        other[rows] = False
        d = rc.store_inputs(*case)
        r = rc.store_ref(d, nh, nkv, hd, rd, pos0)
        a = (d["qkv"], d["cos"], d["sin"], d["kc"], d["vc"], d["vtc"], pos0,
             nh, nkv, rd)
        got = cake_amd.op_kv_store_pr(*a, eps=rc.EPS, decode=decode)
        gq, gk, gv, gvt = got
        qr_, kr_ = r["qrot"], r["krot"][:, rows]
        eq = np.max((np.abs(gq - r["q"]) / np.where(qr_, r["qtol"], 1))[qr_])
        ek = np.max((np.abs(gk - r["kc"])[:, rows] /
                     np.where(kr_, r["ktol"][:, rows], 1))[kr_])
        print(f"{kernel} {case}: q {eq:.3f} K {ek:.3f} of the bound")
        WORST[kernel] = max(WORST[kernel], eq, ek)
        if not (eq <= 1.0 and ek <= 1.0):
            fails.append(f"{case}: q {eq:.3f}, K {ek:.3f} of the bound")
        # pass-through dims: q left in place, K the raw bits
        if not np.array_equal(lc.got_bits(gq[~qr_], False),
                              lr.bf16_bits(r["q"][~qr_])):
            fails.append(f"{case}: q's pass-through dims changed")
        if not np.array_equal(lc.got_bits(gk[:, rows][~kr_], False),
                              lr.bf16_bits(r["kc"][:, rows][~kr_])):
            fails.append(f"{case}: K's pass-through dims are not the raw bits")
        if not np.array_equal(lc.got_bits(gv[:, rows], False),
                              lr.bf16_bits(r["vc"][:, rows])):
            fails.append(f"{case}: V is not the raw bits")
        if not np.array_equal(_bits(gvt[:, :, rows]),
                              _bits(gv[:, rows].transpose(0, 2, 1))):
            fails.append(f"{case}: V^T differs from V")
        for name, g_, was in (("kc", gk[:, other], d["kc"][:, other]),
                              ("vc", gv[:, other], d["vc"][:, other]),
                              ("vtc", gvt[:, :, other],
                               d["vtc"][:, :, other])):
            if not np.array_equal(_bits(g_), _bits(was)):
                fails.append(f"{case}: a {name} slot outside the call changed")
        for _ in range(2):                       # three runs in all
            if not _same(got, cake_amd.op_kv_store_pr(*a, eps=rc.EPS,
                                                      decode=decode)):
                fails.append(f"{case}: a repeat differs")
    # rd == hd through the new entry == the old entry
    cos, sin = rc.tables(rc.STORE_MAX_SEQ, hd)
    a = (d["qkv"], cos, sin, d["kc"], d["vc"], d["vtc"], pos0, nh, nkv)
    old = cake_amd.op_kv_store(*a, eps=rc.EPS, decode=decode)
    new = cake_amd.op_kv_store_pr(*a, hd, eps=rc.EPS, decode=decode)
    if not _same(old, new):
        fails.append("rd == hd differs from op_kv_store")
    assert not fails, "\n".join(fails)


# ---- fused kernel -------------------------------------------------------------
def _check_fused(case, fails):
    nh, nkv, hd, rd, K, pos = case
    kb = cake_amd.linear_dispatch("qkv_rope", 128, K)["kb"]
    kernel = f"qkv_rope_pr KB{kb}"
    other = np.ones(lc.ROPE_MAX_SEQ, dtype=bool)
    other[pos] = False
    for fam in rc.FUSED_FAMILIES:
        d = rc.fused_inputs(fam, *case)
        r = rc.fused_ref(d, nh, nkv, hd, rd, pos)
        a = (d["x"], d["nw"], d["w"], d["cos"], d["sin"], d["kc"], d["vc"],
             d["vtc"], pos, nh, nkv, rd)
        got = cake_amd.op_gemv_qkv_rope_pr(*a, eps=lc.EPS)
        q, rest, kc, vc, vtc = got
        tag = f"{case} {fam}"
        if not np.array_equal(_bits(rest), _bits(np.full_like(
                rest, cake_amd.OP_SENTINEL))):
            fails.append(f"{tag}: the activation row past q was written")
        errs = {}
        for name, g_ in (("q", q), ("k", kc[:, pos])):
            rot = r[name + "_rot"]
            e = np.abs(g_ - r[name]) / r[name + "_bound"]
            errs[name] = np.max(e[rot])
            if d["exact"]:
                if not np.array_equal(lc.got_bits(g_[~rot], False),
                                      lr.bf16_bits(r[name][~rot])):
                    fails.append(f"{tag}: {name}'s pass-through dims differ "
                                 "from RNE_bf16(sum)")
            else:
                errs[name] = max(errs[name], np.max(e[~rot]))
        if d["exact"]:
            if not np.array_equal(lc.got_bits(vc[:, pos], False),
                                  lr.bf16_bits(r["v"])):
                fails.append(f"{tag}: V differs from RNE_bf16(sum)")
        else:
            errs["v"] = np.max(np.abs(vc[:, pos] - r["v"]) / r["v_bound"])
        WORST[kernel] = max(WORST[kernel], *errs.values())
        print(f"{kernel} {tag}: " + " ".join(
            f"{k} {v:.3f}" for k, v in errs.items()) + " of the bound")
        if not all(v <= 1.0 for v in errs.values()):
            fails.append(f"{tag}: {errs} of the bound")
        if not np.array_equal(_bits(vtc[:, :, pos]), _bits(vc[:, pos])):
            fails.append(f"{tag}: V^T column differs from the V row")
        for name, g_, was in (("kc", kc[:, other], d["kc"][:, other]),
                              ("vc", vc[:, other], d["vc"][:, other]),
                              ("vtc", vtc[:, :, other],
                               d["vtc"][:, :, other])):
            if not np.array_equal(_bits(g_), _bits(was)):
                fails.append(f"{tag}: {name} slot other than {pos} changed")
        if not d["exact"]:
            continue
        # the split route (plain GEMV, then the store kernel with rd) agrees
        # bit for bit on V and on the pass-through dims where both round the
        # same exact sums
        raw, _, _ = cake_amd.op_gemv(d["x"][None, :], d["w"], nw=d["nw"],
                                     eps=lc.EPS)
        q2, k2, v2, vt2 = cake_amd.op_kv_store_pr(
            raw, d["cos"], d["sin"], d["kc"], d["vc"], d["vtc"], pos, nh, nkv,
            rd, decode=True)
        if not (np.array_equal(_bits(vc), _bits(v2)) and
                np.array_equal(_bits(vtc), _bits(vt2))):
            fails.append(f"{tag}: V differs from GEMV + store")
        if not (np.array_equal(_bits(q[:, rd:]), _bits(q2[0][:, rd:])) and
                np.array_equal(_bits(kc[:, pos, rd:]),
                               _bits(k2[:, pos, rd:]))):
            fails.append(f"{tag}: pass-through dims differ from GEMV + store")
    return d, a, got


@pytest.mark.parametrize(
    "cases", _groups(rc.fused_cases(), lambda c: c[:3] + c[4:]),
    ids=lambda g: _id(g[0][:3] + g[0][4:]))
def test_qkv_rope_pr(cases):
    fails = []
    for case in cases:
        d, a, got = _check_fused(case, fails)
    for _ in range(2):                           # three runs in all
        if not _same(got, cake_amd.op_gemv_qkv_rope_pr(*a, eps=lc.EPS)):
            fails.append(f"{case}: a repeat differs")
    # rd == hd through the new entry == the old entry (the full-rotation
    # kernel)
    nh, nkv, hd, rd, K, pos = case
    cos, sin = rc.tables(lc.ROPE_MAX_SEQ, hd)
    a = (d["x"], d["nw"], d["w"], cos, sin, d["kc"], d["vc"], d["vtc"], pos,
         nh, nkv)
    old = cake_amd.op_gemv_qkv_rope(*a, eps=lc.EPS)
    new = cake_amd.op_gemv_qkv_rope_pr(*a, hd, eps=lc.EPS)
    if not _same(old, new):
        fails.append("rd == hd differs from op_gemv_qkv_rope")
    assert not fails, "\n".join(fails)
