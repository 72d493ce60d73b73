"""CPU tests of the attention reference and of the GPU op tests' inputs.

Teeth condition: for every shape the GPU tests run, every mutation of the
reference that applies to the shape (a wrong mask edge, a dropped key, a
wrong kv-head) must move the result by MORE than twice the GPU tolerance in at
least one element — otherwise a kernel with that bug would pass.  The four
input families split the work (no single softmax shape can expose every edge
at every context length: a ramp that makes the newest key dominate hides the
oldest, and the other way round), so the condition is asserted per shape
over the families the GPU test runs, and additionally per family for the
edges that family is built for:
    ramp_up   -> causal+1, self_dropped
    ramp_down -> window+1, window-1, oldest_dropped
    peaky     -> mult32_dropped, mult64_dropped, neighbour_kv_head
A shape that fails gets other inputs, never another threshold."""
import numpy as np
import pytest

from oracle import causal_mask, softmax_lastdim
from tests import attn_cases as ac
from tests.attn_ref import MUTATIONS, attn_ref, kv_store_ref, visible_set

DESIGNATED = {
    "ramp_up": ("causal+1", "self_dropped"),
    "ramp_down": ("window+1", "window-1", "oldest_dropped"),
    "peaky": ("mult32_dropped", "mult64_dropped", "neighbour_kv_head"),
}


@pytest.mark.parametrize("S,pos0,window", [
    (1, 0, 0), (5, 0, 3), (7, 45, 0), (33, 45, 40), (4, 64, 1), (9, 20, 9)])
def test_reference_matches_oracle_mask_and_softmax(S, pos0, window):
    rng = np.random.default_rng(S * 1000 + pos0 * 10 + window)
    nh, nkv, hd, max_seq = 4, 2, 16, 96
    q = rng.standard_normal((S, nh, hd))
    kc = rng.standard_normal((nkv, max_seq, hd))
    vc = rng.standard_normal((nkv, max_seq, hd))
    out, A = attn_ref(q, kc, vc, pos0, window)
    n = pos0 + S
    masked = causal_mask(S, n, window or None)
    assert np.array_equal(~masked, visible_set(S, pos0, window, max_seq)[:, :n])
    assert not visible_set(S, pos0, window, max_seq)[:, n:].any()
    for h in range(nh):
        g = h // (nh // nkv)
        s = (q[:, h] @ kc[g, :n].T) / np.sqrt(hd)
        P = softmax_lastdim(np.where(masked, -np.inf, s))
        np.testing.assert_allclose(out[:, h * hd:(h + 1) * hd], P @ vc[g, :n],
                                   rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(A[:, h * hd:(h + 1) * hd],
                                   P @ np.abs(vc[g, :n]), rtol=1e-12,
                                   atol=1e-13)


def test_hooks_change_only_what_they_say():
    S, pos0, window, max_seq = 6, 40, 5, 64
    base = visible_set(S, pos0, window, max_seq)
    assert base.sum(axis=1).tolist() == [5] * S
    kw = MUTATIONS["window+1"](S, pos0, window, max_seq, 4, 2)
    assert kw["vis_hook"](base, None).sum(axis=1).tolist() == [6] * S
    kw = MUTATIONS["causal+1"](S, pos0, window, max_seq, 4, 2)
    new = kw["vis_hook"](base, None)
    assert (new & ~base).sum(axis=1).tolist() == [1] * S
    assert new[0, pos0 + 1] and not base[0, pos0 + 1]
    # a one-key row cannot drop its only key; window 0 has no window edge
    assert MUTATIONS["self_dropped"](1, 0, 0, 32, 2, 1) is None
    assert MUTATIONS["window-1"](4, 0, 0, 32, 2, 1) is None
    assert MUTATIONS["window-1"](4, 8, 1, 32, 2, 1) is None
    assert MUTATIONS["neighbour_kv_head"](4, 0, 0, 32, 2, 1) is None


def test_store_reference_is_plain_rope():
    rng = np.random.default_rng(3)
    nh, nkv, hd, max_seq, S, pos0 = 2, 1, 8, 32, 3, 5
    qkv = rng.standard_normal((S, (nh + 2 * nkv) * hd))
    ang = rng.standard_normal((max_seq, hd // 2))
    z = np.full((nkv, max_seq, hd), 7.0)
    q, kc, vc, vtc, _, _ = kv_store_ref(qkv, np.cos(ang), np.sin(ang), pos0,
                                        nh, nkv, z, z, z.transpose(0, 2, 1))
    rows = qkv.reshape(S, nh + 2, hd)
    x1, x2 = rows[1, 0, :4], rows[1, 0, 4:]
    c, s = np.cos(ang[6]), np.sin(ang[6])
    np.testing.assert_allclose(q[1, 0], np.r_[x1 * c - x2 * s,
                                              x2 * c + x1 * s])
    assert np.array_equal(vc[0, 5:8], rows[:, 3])
    assert np.array_equal(vtc[0, :, 5:8], rows[:, 3].T)
    untouched = np.r_[0:5, 8:max_seq]
    assert (kc[:, untouched] == 7.0).all() and (vc[:, untouched] == 7.0).all()
    assert (vtc[:, :, untouched] == 7.0).all()


def test_case_lists_cover_every_listed_value():
    """The pruned cross products still contain every shape value, variant
    and geometry the GPU tests are meant to reach."""
    mf = ac.PF_MFMA_CASES
    assert {c[2] for _, c in mf} == {1, 31, 32, 33, 129, 257}
    assert {c[3] for _, c in mf} == {0, 1, 45, 64}
    assert {c[4] for _, c in mf} == {0, 1, 32, 33, 40}
    assert {c[:2] for _, c in mf} == {(2, 1), (4, 2), (8, 1)}
    assert any(c[3] + c[2] == c[5] for _, c in mf)
    variants = {v for v, _ in mf}
    assert len(variants) == 9
    must = {(33, 45, 40), (257, 0, 0), (129, 64, 33)}
    for v in variants:
        assert must <= {c[2:5] for vv, c in mf if vv == v}, v
    assert all(c[3] + c[2] <= c[5] and c[5] % 32 == 0 for _, c in mf)
    ge = ac.PF_GENERIC_CASES
    assert {c[0] for c in ge} == {8, 40, 64, 96}
    for hd in (8, 40, 64, 96):
        assert {c[5] for c in ge if c[0] == hd} == {0, 1, 24}
    assert {c[3] for c in ge} == {1, 3, 4, 5, 77}
    assert {c[4] for c in ge} == {0, 45}
    for cases, nchunks in ((ac.DEC_G_CASES, {1, 2, 4, 8, 24, 32, 48, 64}),
                           (ac.DEC_F_CASES, {2, 8, 12, 16})):
        for cfg in {c[:3] for c in cases}:
            mine = [c for c in cases if c[:3] == cfg]
            assert {c[3] for c in mine} == set(ac.DEC_N), cfg
            assert {c[4] for c in mine} == nchunks, cfg
            assert {c[5] for c in mine} == set(ac.DEC_WINDOWS), cfg
    assert {c[:3] for c in ac.DEC_G_CASES} == {
        (4, 1, 128), (8, 1, 128), (8, 2, 128), (2, 1, 128), (2, 2, 128)}
    assert {c[:3] for c in ac.DEC_F_CASES} == {
        (3, 1, 128), (6, 2, 128), (4, 2, 8), (4, 2, 40), (4, 2, 64)}


# ---- teeth ----------------------------------------------------------------
def _shapes():
    """(tol, nh, nkv, hd, S, pos0, window, max_seq, decode), deduplicated."""
    out = []
    for _, (nh, nkv, S, pos0, w, ms) in ac.PF_MFMA_CASES:
        out.append((ac.TOL_MFMA, nh, nkv, 128, S, pos0, w, ms, False))
    for hd, nh, nkv, S, pos0, w in ac.PF_GENERIC_CASES:
        out.append((ac.TOL_F32P, nh, nkv, hd, S, pos0, w, 128, False))
    for nh, nkv, hd, n, _, w in ac.DEC_G_CASES + ac.DEC_F_CASES:
        out.append((ac.TOL_F32P, nh, nkv, hd, 1, n - 1, w,
                    ac.decode_max_seq(n), True))
    return sorted(set(out))


def _shape_id(s):
    tol, nh, nkv, hd, S, pos0, w, ms, dec = s
    return (f"{'dec' if dec else 'pf'}-hd{hd}-nh{nh}kv{nkv}-S{S}-p{pos0}"
            f"-w{w}-tol{int(-np.log2(tol))}")


@pytest.mark.parametrize("shape", _shapes(), ids=_shape_id)
def test_gpu_case_inputs_have_teeth(shape):
    tol, nh, nkv, hd, S, pos0, window, max_seq, decode = shape
    muts = {name: make(S, pos0, window, max_seq, nh, nkv)
            for name, make in MUTATIONS.items()}
    muts = {k: v for k, v in muts.items() if v is not None}
    margin = {name: {} for name in muts}
    for fam in ac.FAMILIES:
        q, kc, vc = ac.make_inputs(fam, nh, nkv, hd, max_seq, S, pos0, window,
                                   decode)
        ref, A = attn_ref(q, kc, vc, pos0, window)
        for name, kw in muts.items():
            bad, _ = attn_ref(q, kc, vc, pos0, window, **kw)
            margin[name][fam] = float(
                np.max(np.abs(bad - ref) / (tol * A + ac.ABS_EPS)))
    for name, per_fam in margin.items():
        # margin is err / tol: > 2 means the bug fails the GPU assertion
        # with a factor two to spare
        assert max(per_fam.values()) > 2.0, (name, per_fam)
        for fam, names in DESIGNATED.items():
            if name in names:
                assert per_fam[fam] > 2.0, (name, fam, per_fam)
