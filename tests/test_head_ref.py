"""CPU tests of the head references and of the GPU tests' inputs
(tests/head_cases.py): the extremes table re-derived in integers, the
conditions the GPU assertions rest on (unique near-top sets, exact conversion
edges), the teeth of every GPU case family (each named defect must move the
reference past what the GPU test allows, on the GPU test's own inputs), and
the argument checks of the two op entries (which run before any device
call)."""
import numpy as np
import pytest

import cake_amd
from tests import head_cases as hc
from tests import sampling_ref as sr


# ---- the uniform stream -----------------------------------------------------
def test_extremes_table_rederived_in_integers():
    for k, (seed, draw, i) in hc.extreme_rows():
        assert i < hc.EXTREMES_V
        assert hc.hash_k(seed, draw, i) == k, (k, seed, draw, i)
    seed, draw, i = hc.POISON_PRODUCT
    assert i < hc.PRODUCT_V and hc.hash_k(seed, draw, i) == hc.K_TOP
    assert set(hc.EXTREMES) == {hc.K_TOP, hc.K_TOP - 1, hc.K_TOP - 2,
                                hc.K_TOP - 3, 0}


def test_contract_u_is_exact_in_f32_and_inside_the_open_interval():
    for k in (0, 1, hc.K_TOP - 2, hc.K_TOP - 1, hc.K_TOP):
        u = (min(k, hc.K_TOP - 1) + 1) * 2.0 ** -24
        assert 0 < u < 1 and float(np.float32(u)) == u
        assert np.isfinite(hc.gumbel_of_k(k))
    assert hc.gumbel_of_k(hc.K_TOP) == hc.gumbel_of_k(hc.K_TOP - 1)
    # the defect this replaces: 16777217 is not an f32, the factor was 2^-24
    assert np.float32(16777217.0) == np.float32(16777216.0)
    assert (np.float32(hc.K_TOP) + np.float32(1)) * (
        np.float32(1) / np.float32(16777217.0)) == np.float32(1.0)


def test_numpy_noise_matches_the_integer_derivation():
    for k, (seed, draw, i) in hc.extreme_rows():
        g = hc.noise(seed, draw, hc.EXTREMES_V)
        assert np.isfinite(g).all()
        assert g[i] == hc.gumbel_of_k(k)
        assert sr.gumbel(seed, draw, hc.EXTREMES_V)[i] == g[i]
    ids = hc.sweep_ids(5)
    g = hc.noise(hc.SWEEP_SEED, hc.SWEEP_DRAW, hc.SWEEP_V)
    for i in ids[::37]:
        assert g[i] == hc.gumbel_of_k(
            hc.hash_k(hc.SWEEP_SEED, hc.SWEEP_DRAW, int(i)))


def test_sweep_covers_512_ids_one_per_partition():
    ids = [hc.sweep_ids(o) for o in hc.SWEEP_OFFSETS]
    assert sum(len(a) for a in ids) >= 512
    allids = np.concatenate(ids)
    assert len(set(allids)) == allids.size and allids.max() < hc.SWEEP_V
    sp = hc.spans(hc.SWEEP_V)
    for a in ids:
        parts = [p for p, (s, e) in enumerate(sp) for i in a if s <= i < e]
        assert len(parts) == len(set(parts)) == len(a)


# ---- greedy: the reference itself, and its teeth ----------------------------
def _greedy(V):
    return hc.greedy_cases(V)


def test_greedy_reference_follows_the_contract():
    want = {"max@first", "max@last", "max@span-1", "max@span",
            "max@lastpart_first", "tie_stride", "tie_threads", "tie_parts",
            "tie_parts_late", "all_equal", "negzero_first", "inf_pair",
            "all_neginf", "all_nan", "nan_but_one", "nan_neginf_mix",
            "nan_before_max"}
    seen = set()
    for V in hc.GREEDY_V:
        for name, x in _greedy(V):
            seen.add(name)
            assert x.dtype == np.float32 and x.size == V
            r = hc.argmax_ref(x)
            assert 0 <= r["token"] < V
            ok = ~np.isnan(x)
            if ok.any() and x[ok].max() > -np.inf:
                # np.argmax sees NaN as the largest: mask it out first
                assert r["token"] == int(np.argmax(np.where(ok, x, -np.inf)))
            else:
                assert r["token"] == 0, (V, name)
    assert seen == want
    x = dict(_greedy(257))["negzero_first"]
    assert np.signbit(x[hc.argmax_ref(x)["token"]])
    # spans: an empty tail below 256 entries and at 257 (span 2)
    assert sum(e > s for s, e in hc.spans(63)) == 63
    assert sum(e > s for s, e in hc.spans(257)) == 129
    assert hc.spans(151936)[255] == (255 * 594, 151936)


def greedy_observation(x, mut=None):
    """What the GPU test compares, as one tuple: the token and the partial
    winners of the spans that have one."""
    r = hc.argmax_ref(x, mut)
    return r["token"], tuple(r["pidx"])


@pytest.mark.parametrize("mut", hc.GREEDY_MUTANTS)
def test_greedy_teeth(mut):
    """Every defect changes the token or a partial winner of some case; the
    span and reduce defects do so at the product vocabulary too."""
    hit = {V: [n for n, x in _greedy(V)
               if greedy_observation(x) != greedy_observation(x, mut)]
           for V in hc.GREEDY_V}
    assert any(hit.values()), mut
    assert hit[hc.PRODUCT_V], mut
    # ... and the token alone moves somewhere
    assert any(hc.argmax_ref(x)["token"] != hc.argmax_ref(x, mut)["token"]
               for V in hc.GREEDY_V for _, x in _greedy(V)), mut


# ---- Gumbel value / poisoned token / draw tokens ---------------------------
def _value_points():
    """(seed, draw, V, id) of every Gumbel value the GPU test measures."""
    pts = [(s, d, hc.EXTREMES_V, i) for _, (s, d, i) in hc.extreme_rows()]
    pts += [(hc.SWEEP_SEED, hc.SWEEP_DRAW, hc.SWEEP_V, int(i))
            for o in hc.SWEEP_OFFSETS for i in hc.sweep_ids(o)]
    return pts


def test_planted_zero_isolates_the_noise():
    """With -1e30 elsewhere the maximum of the scores is the planted id and
    its score is the noise itself, in float64 and in f32 (-1e30 + G rounds
    to -1e30)."""
    seed, draw, i = hc.EXTREMES[0][0]
    x = hc.planted_zero(hc.EXTREMES_V, [i])
    sc = hc.scores(x, 1.0, seed, draw)
    assert int(np.argmax(sc)) == i and sc[i] == hc.gumbel_of_k(0)
    assert np.float32(hc.GUMBEL_LOW) + np.float32(20.0) == hc.GUMBEL_LOW
    ids = hc.sweep_ids(16)
    sc = hc.scores(hc.planted_zero(hc.SWEEP_V, ids), 1.0, hc.SWEEP_SEED,
                   hc.SWEEP_DRAW)
    r = hc.argmax_ref(sc)
    assert set(r["pidx"][r["pidx"] != hc.NONE]) >= set(ids)


@pytest.mark.parametrize("mut", ("u_can_be_one", "step_off_by_one",
                                 "index_off_by_one"))
def test_gumbel_value_teeth(mut):
    moved = 0
    for seed, draw, V, i in _value_points():
        ref = hc.noise(seed, draw, V)[i]
        got = hc.noise(seed, draw, V, mut)[i]
        moved += not abs(got - ref) <= hc.gumbel_bound(ref)
    assert moved >= (3 if mut == "u_can_be_one" else 100), (mut, moved)


def test_poisoned_token_teeth():
    """Unclamped u makes the poisoned id win every case; the contract never
    does, and its near-top set excludes the id."""
    for V, seed, draw, i in hc.poison_cases():
        x = hc.poison_logits(V, i)
        bad = hc.scores(x, 1.0, seed, draw, "u_can_be_one")
        assert hc.argmax_ref(bad)["token"] == i and np.isinf(bad[i])
        r = hc.draw_step_ref(x, 1.0, seed, draw)
        assert i not in r["near"] and r["near"].size >= 1


@pytest.mark.parametrize("case", hc.DRAW_CASES, ids=str)
def test_draw_cases_have_unique_near_top_sets_and_teeth(case):
    V, T, seed, first = case
    ref = hc.draw_reference(*case)
    single = sum(near.size == 1 for near, *_ in ref)
    assert single >= 0.99 * hc.DRAW_STEPS, single
    assert len({top for _, top, *_ in ref}) > hc.DRAW_STEPS // 2
    l = hc.draw_logits(V)
    for mut in ("step_off_by_one", "index_off_by_one", "temp_multiplied"):
        out = 0
        for j, (near, *_r) in enumerate(ref):
            tok = hc.argmax_ref(hc.scores(l, T, seed, first + j, mut))["token"]
            out += tok not in near
        # one token outside its near-top set fails the GPU test
        assert out >= 1, (mut, out)


def test_every_gumbel_mutant_has_a_teeth_test():
    assert set(hc.GUMBEL_MUTANTS) == {"u_can_be_one", "step_off_by_one",
                                      "index_off_by_one", "temp_multiplied"}


# ---- bookkeeping ------------------------------------------------------------
def test_bookkeeping_reference_and_teeth():
    toks = np.arange(40, 40 + hc.BOOK_STEPS, dtype=np.uint32)
    img, step, pos = hc.book_ref(toks, hc.BOOK_FIRST, True, 1)
    assert step == 8 and pos == 5
    assert (img[:3] == hc.SENT_BITS).all() and (img[3:8] == toks).all()
    assert hc.book_ref(toks, hc.BOOK_FIRST, True, 0)[2] == 0
    assert hc.book_ref(toks, hc.BOOK_FIRST, False, 1) == (None, 3, 5)
    for mut in hc.BOOK_MUTANTS:
        bad = hc.book_ref(toks, hc.BOOK_FIRST, True, 1, mut)[0]
        assert not np.array_equal(bad, img), mut
    # the sentinel is no token of the bookkeeping vocabulary, and the five
    # steps draw more than one token, so a ring slot shows which step wrote it
    assert hc.SENT_BITS >= hc.BOOK_V
    l = hc.book_logits()
    ref = [hc.draw_step_ref(l, hc.BOOK_T, hc.BOOK_SEED, s)
           for s in range(hc.BOOK_FIRST, hc.BOOK_FIRST + hc.BOOK_STEPS)]
    assert all(r["near"].size == 1 for r in ref)
    assert len({r["top"] for r in ref}) == hc.BOOK_STEPS


# ---- embedding --------------------------------------------------------------
def test_conversion_edges_round_as_listed():
    t = hc.embed_table(hc.EMBED_VT, 72)
    bits = hc.table_bits(t)
    n = len(hc.EDGE_WORDS)
    assert n <= 72
    assert list(bits[hc.EDGE_ROW][:n]) == [b for _, b in hc.EDGE_WORDS]
    assert list(t[hc.EDGE_ROW][:n].view(np.uint32)) == [
        a for a, _ in hc.EDGE_WORDS]
    assert not t[hc.ZERO_ROW].any()
    # the other rows are not bf16-exact: the upload has to round them
    assert ((t[0].view(np.uint32) & 0xFFFF) != 0).mean() > 0.9
    Vt, H = hc.EMBED_BIG
    assert Vt * H > 2048 * 256


def _embed_all_cases():
    for Vt, H, S in hc.embed_rows_cases():
        yield Vt, H, hc.embed_ids(Vt, S)
    for Vt, H, i, _ in hc.embed_token_cases():
        yield Vt, H, np.array([i])


def test_embed_ids_cover_the_issue():
    ids = list(hc.embed_ids(hc.EMBED_VT, 5))
    assert 0 in ids and hc.EMBED_VT - 1 in ids and hc.EDGE_ROW in ids
    assert hc.ZERO_ROW in ids and len(set(ids)) < len(ids)
    assert list(hc.embed_ids(hc.EMBED_VT, 1)) == [hc.EDGE_ROW]


@pytest.mark.parametrize("mut", ("embed_row_next", "embed_tail_dropped"))
def test_embed_teeth(mut):
    """Bit-equality is the GPU assertion: the defect flips a word in every
    rows case."""
    tables = {}
    for Vt, H, S in hc.embed_rows_cases():
        t = tables.setdefault((Vt, H), hc.embed_table(Vt, H))
        ids = hc.embed_ids(Vt, S)
        assert not np.array_equal(hc.embed_ref(t, ids),
                                  hc.embed_ref(t, ids, mut)), (mut, Vt, H, S)


@pytest.mark.parametrize("mut", ("nscale_no_eps", "nscale_sum_not_mean"))
def test_nscale_teeth(mut):
    for H in hc.EMBED_H:
        t = hc.embed_table(hc.EMBED_VT, H)
        moved = 0
        for i in (0, hc.EMBED_VT - 1, hc.ZERO_ROW):
            ref = hc.nscale_ref(t, i, hc.EPS)
            got = hc.nscale_ref(t, i, hc.EPS, mut)
            moved += not abs(got - ref) <= 2 * hc.TOL_F32 * ref
        assert moved, (mut, H)
    t = hc.embed_table(hc.EMBED_VT, 8)
    assert hc.nscale_ref(t, hc.ZERO_ROW, hc.EPS) == 1 / np.sqrt(hc.EPS)


def test_every_listed_mutant_is_exercised():
    assert set(hc.EMBED_MUTANTS) == {"embed_row_next", "embed_tail_dropped",
                                     "nscale_no_eps", "nscale_sum_not_mean"}
    assert set(hc.GREEDY_MUTANTS) == {"tie_last", "span_floor",
                                      "part_tail_dropped",
                                      "fin_first_half_only", "nan_wins"}


# ---- argument checks run before any device call ----------------------------
def test_op_entries_reject_bad_arguments_without_a_device():
    E = cake_amd.CakeHipError
    x = np.zeros(8, np.float32)
    for kw in (dict(steps=0), dict(steps=8193), dict(first_step=-1),
               dict(first_step=(1 << 20) + 1), dict(advance_pos=2),
               dict(temperature=float("nan"))):
        with pytest.raises(E, match="op_argmax"):
            cake_amd.op_argmax(x, **kw)
    with pytest.raises(E, match="op_argmax: V"):
        cake_amd.op_argmax(np.zeros(0, np.float32))
    t = np.zeros((7, 8), np.float32)
    with pytest.raises(E, match="multiple of 8"):
        cake_amd.op_embed(np.zeros((7, 12), np.float32), [0])
    with pytest.raises(E, match="multiple of 8"):
        cake_amd.op_embed(np.zeros((2, 16392), np.float32), [0])
    with pytest.raises(E, match="outside the table"):
        cake_amd.op_embed(t, [0, 7])
    with pytest.raises(E, match="S 2"):
        cake_amd.op_embed(t, [0, 1], mode="token")
    with pytest.raises(E, match="S 0"):
        cake_amd.op_embed(t, [])


def test_engine_create_rejects_hidden_sizes_off_the_8_grid():
    """op_embed mirrors engine create: H % 8 != 0 is refused there too, so
    there is no H = 12 case."""
    cfg = dict(
        model_type="llama", hidden_size=12, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=4,
        num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-5,
        rope_theta=10000.0, max_position_embeddings=128,
        tie_word_embeddings=False)
    with pytest.raises(cake_amd.CakeHipError, match="multiples of 8"):
        cake_amd.Engine(cfg, max_seq=32, max_batch_tokens=8)
