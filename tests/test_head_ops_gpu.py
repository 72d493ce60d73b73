"""GPU tests of the two ends of the decode step against the float64
references of tests/head_cases.py: launch_argmax (greedy token and the 256
partials exactly; ring / step / pos bookkeeping; the Gumbel noise measured
directly; draw tokens within the derived bound), the Gumbel draw of
launch_sample with the selectors off, and the embedding gathers with the
f32 <-> bf16 conversion kernels (bit-exact) and the norm chain's nscale.

A token is only ever looked at as a number here: the argmax contract (always
< V, 0 when nothing is greater than -inf) is tested through the op entries,
never through an engine that would dereference it."""
import numpy as np
import pytest

import cake_amd
from tests import head_cases as hc

pytestmark = pytest.mark.gpu

SENT = np.uint32(hc.SENT_BITS)


def _guards_intact(r):
    assert (r["part_guards"] == SENT).all()
    if r["ring"] is not None:
        assert (r["ring_guards"] == SENT).all()


# ---- greedy -----------------------------------------------------------------
@pytest.mark.parametrize("V", hc.GREEDY_V)
def test_greedy_token_and_partials_exact(V):
    """temperature 0: the token equals the reference; pidx[p] is the
    reference winner of span p and pval[p] is bit-equal to that logit; spans
    without a winner (empty, or all NaN) hold -inf and so cannot win."""
    for name, x in hc.greedy_cases(V):
        ref = hc.argmax_ref(x)
        r = cake_amd.op_argmax(x, temperature=0.0, first_step=2)
        _guards_intact(r)
        tok = int(r["tokens"][0])
        assert tok < V, (name, tok)
        assert tok == ref["token"], (name, tok, ref["token"])
        assert list(r["ring"][2:]) == [tok] and (r["ring"][:2] == SENT).all()
        assert (r["pos"], r["step"]) == (1, 3)
        has = ref["pidx"] != hc.NONE
        assert np.array_equal(r["pidx"][has], ref["pidx"][has]), name
        want = x[ref["pidx"][has]].view(np.uint32)
        assert np.array_equal(r["pval"][has].view(np.uint32), want), name
        assert np.isneginf(r["pval"][~has]).all(), name


def test_greedy_ignores_the_seed_and_the_step():
    x = dict(hc.greedy_cases(4099))["max@span"]
    a = cake_amd.op_argmax(x, temperature=0.0, seed=1, first_step=0)
    b = cake_amd.op_argmax(x, temperature=-1.0, seed=2, first_step=9, steps=3)
    assert list(b["tokens"]) == [int(a["tokens"][0])] * 3


# ---- bookkeeping ------------------------------------------------------------
@pytest.mark.parametrize("advance_pos", (0, 1))
def test_ring_step_and_pos_bookkeeping(advance_pos):
    """5 sampled steps from step 3: ring slots 3..7 hold the tokens of steps
    3..7 (all different), slots 0..2 and the guards are untouched, step ends
    at 8 and pos advanced by 5 * advance_pos."""
    l = hc.book_logits()
    steps = range(hc.BOOK_FIRST, hc.BOOK_FIRST + hc.BOOK_STEPS)
    want = [hc.draw_step_ref(l, hc.BOOK_T, hc.BOOK_SEED, s)["top"]
            for s in steps]
    r = cake_amd.op_argmax(l, temperature=hc.BOOK_T, seed=hc.BOOK_SEED,
                           first_step=hc.BOOK_FIRST, steps=hc.BOOK_STEPS,
                           advance_pos=advance_pos)
    _guards_intact(r)
    assert list(r["tokens"]) == want
    img, step, pos = hc.book_ref(r["tokens"], hc.BOOK_FIRST, True,
                                 advance_pos)
    assert np.array_equal(r["ring"], img)
    assert (r["step"], r["pos"]) == (step, pos) == (8, 5 * advance_pos)


def test_null_ring_leaves_the_step_and_the_noise_in_place():
    l = hc.book_logits()
    want = hc.draw_step_ref(l, hc.BOOK_T, hc.BOOK_SEED, hc.BOOK_FIRST)["top"]
    r = cake_amd.op_argmax(l, temperature=hc.BOOK_T, seed=hc.BOOK_SEED,
                           first_step=hc.BOOK_FIRST, steps=hc.BOOK_STEPS,
                           ring=False)
    _guards_intact(r)
    assert r["ring"] is None
    assert list(r["tokens"]) == [want] * hc.BOOK_STEPS
    assert (r["step"], r["pos"]) == (hc.BOOK_FIRST, hc.BOOK_STEPS)


# ---- Gumbel value, measured directly ----------------------------------------
def _measure(V, ids, seed, draw):
    """Device noise at `ids` (one per partition) of draw index `draw`."""
    ids = np.asarray(ids)
    r = cake_amd.op_argmax(hc.planted_zero(V, ids), temperature=1.0,
                           seed=seed, first_step=draw)
    _guards_intact(r)
    part = ids // hc.span_of(V)
    assert np.array_equal(r["pidx"][part], ids)
    assert int(r["tokens"][0]) in ids
    return r["pval"][part].astype(np.float64)


def _ratio(got, ref):
    assert np.isfinite(got).all(), got
    return np.abs(got - ref) / hc.gumbel_bound(ref)


def test_gumbel_value_at_the_extremes():
    """|G_dev - G_ref| <= 2^-18 (1 + |G_ref|) at the hash bits 2^24 - 1 ..
    2^24 - 4 and 0; every value finite."""
    worst = 0.0
    for k, (seed, draw, i) in hc.extreme_rows():
        got = _measure(hc.EXTREMES_V, [i], seed, draw)
        ref = hc.gumbel_of_k(k)
        q = float(_ratio(got, ref)[0])
        print(f"k={k:#x} ({seed},{draw},{i}): dev {got[0]!r} ref {ref!r} "
              f"ratio {q:.4f}")
        worst = max(worst, q)
    print(f"gumbel extremes: largest |err| / bound = {worst:.4f}")
    assert worst <= 1.0


def test_gumbel_value_sweep():
    """One id per partition, three launches of one draw: > 512 ids."""
    g = hc.noise(hc.SWEEP_SEED, hc.SWEEP_DRAW, hc.SWEEP_V)
    worst, n = 0.0, 0
    for off in hc.SWEEP_OFFSETS:
        ids = hc.sweep_ids(off)
        q = _ratio(_measure(hc.SWEEP_V, ids, hc.SWEEP_SEED, hc.SWEEP_DRAW),
                   g[ids])
        worst, n = max(worst, float(q.max())), n + ids.size
    print(f"gumbel sweep: {n} ids, largest |err| / bound = {worst:.4f}")
    assert n >= 512 and worst <= 1.0


# ---- poisoned token ---------------------------------------------------------
def _sample_off(x, T, seed, first, draws=1):
    toks, kept, _ = cake_amd.op_sample(x, T, seed=seed, first_draw=first,
                                       draws=draws)
    assert kept == x.size
    return toks


@pytest.mark.parametrize("case", hc.poison_cases(), ids=str)
def test_hash_bits_all_ones_do_not_pick_the_token(case):
    """Zeros everywhere, -1e4 at the id whose hash bits are all ones: both
    samplers return a token of the reference near-top set, never that id."""
    V, seed, draw, i = case
    x = hc.poison_logits(V, i)
    near = hc.draw_step_ref(x, 1.0, seed, draw)["near"]
    a = int(cake_amd.op_argmax(x, temperature=1.0, seed=seed,
                               first_step=draw)["tokens"][0])
    b = int(_sample_off(x, 1.0, seed, draw)[0])
    print(f"{case}: op_argmax {a} op_sample {b} near-top {list(near)}")
    for tok in (a, b):
        assert tok != i
        assert tok in near


# ---- draw tokens ------------------------------------------------------------
@pytest.mark.parametrize("case", hc.DRAW_CASES, ids=str)
def test_draw_tokens_within_the_bound_and_equal_between_the_samplers(case):
    """64 consecutive steps: every token's reference score is within 2 tol of
    the reference maximum, and launch_argmax and launch_sample (selectors
    off) return the same tokens at step == draw."""
    V, T, seed, first = case
    l = hc.draw_logits(V)
    ref = hc.draw_reference(*case)
    r = cake_amd.op_argmax(l, temperature=T, seed=seed, first_step=first,
                           steps=hc.DRAW_STEPS)
    _guards_intact(r)
    toks = r["tokens"]
    assert np.array_equal(r["ring"][first:], toks)
    assert np.array_equal(_sample_off(l, T, seed, first, hc.DRAW_STEPS), toks)
    off = [(j, int(t)) for j, (t, (near, *_)) in enumerate(zip(toks, ref))
           if t not in near]
    assert not off, off


# ---- embedding --------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16


_tables = {}


def _table(Vt, H):
    if (Vt, H) not in _tables:
        _tables[(Vt, H)] = hc.embed_table(Vt, H)
    return _tables[(Vt, H)]


def _plain(a):
    assert (np.ascontiguousarray(a).view(np.uint32) & 0xFFFF == 0).all()


@pytest.mark.parametrize("case", hc.embed_rows_cases(), ids=str)
def test_embed_rows_bit_exact(case):
    Vt, H, S = case
    t, ids = _table(Vt, H), hc.embed_ids(Vt, S)
    out, guards, ns, nsg = cake_amd.op_embed(t, ids, "rows")
    _plain(out)
    assert np.array_equal(_bits(out), hc.embed_ref(t, ids))
    assert (guards == cake_amd.OP_SENTINEL).all()
    assert ns == cake_amd.OP_SENTINEL and (nsg == cake_amd.OP_SENTINEL).all()


@pytest.mark.parametrize("case", hc.embed_token_cases(), ids=str)
def test_embed_token_bit_exact_and_nscale(case):
    Vt, H, i, want_ns = case
    t = _table(Vt, H)
    out, guards, ns, nsg = cake_amd.op_embed(
        t, [i], "token_nscale" if want_ns else "token", eps=hc.EPS)
    _plain(out)
    assert np.array_equal(_bits(out), hc.embed_ref(t, [i]))
    assert (guards == cake_amd.OP_SENTINEL).all()
    assert (nsg == cake_amd.OP_SENTINEL).all()
    if not want_ns:
        assert ns == cake_amd.OP_SENTINEL
    elif i != hc.EDGE_ROW:        # the edge row holds inf and NaN
        ref = hc.nscale_ref(t, i, hc.EPS)
        print(f"{case}: nscale {ns!r} ref {ref!r}")
        assert abs(float(ns) - ref) <= hc.TOL_F32 * ref
        if i == hc.ZERO_ROW:
            assert ref == 1 / np.sqrt(hc.EPS)
