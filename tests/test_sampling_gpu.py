"""GPU tests of the on-device sampler (kernels_sample.hip) against the float64
reference of tests/sampling_ref.py: the kept-set size and tau exactly, the
penalised argmax exactly, draws by support / chi-square / reproducibility,
and the engine-level plumbing (graphs, draw counter, history, reset).

The engine-level case of "repeat_last_n shorter than the history" is
test_engine_greedy_penalty_stepwise; the op entry penalises all it is given.
"""
import json

import numpy as np
import pytest

import cake_amd
from tests import sampling_cases as sc
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu

CHI_BOUND = 31.0  # the 1e-6 tail of chi-square at 3 degrees of freedom


# ---------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("V", sc.VS)
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_op_kept_and_tau_exact(family, V):
    """top-k alone (k in 1, 2, 40, V-1, V, V+7), top-p alone, k-then-p, each
    with and without penalty: kept and tau equal the reference exactly, and
    the drawn token lies in the reference kept set."""
    logits, _ = sc.make_logits(family, V)
    for i, c in enumerate(sc.cases(family, V)):
        ref = sc.reference(family, V, i)
        toks, kept, tau = cake_amd.op_sample(
            logits, sc.T, top_k=c["top_k"], top_p=c["top_p"],
            repeat_penalty=c["penalty"], history=c["history"], seed=11,
            first_draw=i, draws=1)
        print(f"{family} V={V} {c['name']}: kept {kept} (ref {ref['kept']}) "
              f"tau {tau!r} (ref {ref['tau']!r})")
        assert kept == ref["kept"], c["name"]
        assert tau == ref["tau"], c["name"]
        assert ref["mask"][toks[0]], c["name"]


@pytest.mark.parametrize("V", [63, 4099, 151936])
def test_op_tie_rule(V):
    x, k, kept_ref, tau_ref = sc.tie_case(V)
    _, kept, tau = cake_amd.op_sample(x, sc.T, top_k=k)
    assert (kept, tau) == (kept_ref, tau_ref)
    eq = np.full(V, -3.25, dtype=np.float32)
    for kw in (dict(top_k=7), dict(top_p=0.5), dict(top_k=7, top_p=0.5)):
        toks, kept, tau = cake_amd.op_sample(eq, sc.T, draws=4, **kw)
        assert kept == V and tau == np.float32(-3.25)
        assert (toks < V).all()


@pytest.mark.parametrize("V", sc.VS)
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_op_greedy_penalty_exact(family, V):
    """temperature <= 0: the token is the first-index argmax of the penalised
    logits (duplicated ids, ids 0 and V-1, a zero logit, negative logits);
    nothing is dropped, tau is the smallest penalised logit."""
    logits, _ = sc.make_logits(family, V)
    hist = sc.history_for(family, V)
    for pen in (sc.PENALTY, 4.0, 0.5):
        lp = sr.penalise(logits, pen, hist)
        for temp in (0.0, -1.0):
            toks, kept, tau = cake_amd.op_sample(
                logits, temp, top_k=3, top_p=0.5, repeat_penalty=pen,
                history=hist, draws=2)
            assert list(toks) == [sr.greedy_token(lp)] * 2
            assert kept == V and tau == lp.min()


def test_op_penalty_moves_the_argmax():
    x = np.array([0.0, -0.5, 3.0, 2.9, -4.0, 2.95], dtype=np.float32)
    for hist, want in (([2], 5), ([2, 5, 2], 3), ([2, 5, 3], 2),
                       ([2, 3, 5, 2, 3, 5, 0, 4], 2)):
        lp = sr.penalise(x, 1.1, hist)
        assert sr.greedy_token(lp) == want
        toks, _, _ = cake_amd.op_sample(x, 0.0, repeat_penalty=1.1,
                                        history=hist)
        assert toks[0] == want
    # the zero logit stays zero and wins over penalised negatives
    z = np.array([-1.0, 0.0, -2.0], dtype=np.float32)
    assert cake_amd.op_sample(z, 0.0, repeat_penalty=2.0,
                              history=[1, 0])[0][0] == 1


@pytest.mark.parametrize("V", [1000, 4099])
@pytest.mark.parametrize("seed", [1, 2, 3, 299792458])
def test_op_draws_distribution(V, seed):
    """4096 consecutive draws on the .4/.3/.2/.1 support: every token in the
    support, chi-square under the 1e-6 tail bound."""
    x, ids, probs = sc.chi_case(V)
    toks, kept, _ = cake_amd.op_sample(x, sc.T, top_k=4, seed=seed,
                                       draws=4096)
    assert kept == 4
    assert np.isin(toks, ids).all()
    chi = sr.chi_square(toks, ids, probs)
    ref_chi = sr.chi_square(sr.draws_on_support(x, ids, sc.T, seed, 0, 4096),
                            ids, probs)
    print(f"V={V} seed={seed}: chi2 device {chi:.3f} reference {ref_chi:.3f}")
    assert chi < CHI_BOUND


def test_op_draws_membership_deep_set():
    """A kept set of 200 (plateau, top-p) and one cut by k then p: all 4096
    draws stay inside the reference kept set."""
    V = 4099
    logits, _ = sc.make_logits("plateau", V)
    for i, c in enumerate(sc.cases("plateau", V)):
        if c["name"] not in ("p@199", "k40p@20+pen"):
            continue
        ref = sc.reference("plateau", V, i)
        toks, kept, _ = cake_amd.op_sample(
            logits, sc.T, top_k=c["top_k"], top_p=c["top_p"],
            repeat_penalty=c["penalty"], history=c["history"], seed=9,
            draws=4096)
        assert kept == ref["kept"]
        assert ref["mask"][toks].all()
        assert np.unique(toks).size > ref["kept"] // 2


def test_op_draws_reproducible_and_seeded():
    V = 4099
    x, _ = sc.make_logits("plateau", V)
    kw = dict(top_k=150, top_p=0.9, repeat_penalty=1.2, history=[1, 2, 1])
    a = cake_amd.op_sample(x, sc.T, seed=5, first_draw=3, draws=256, **kw)
    b = cake_amd.op_sample(x, sc.T, seed=5, first_draw=3, draws=256, **kw)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    c = cake_amd.op_sample(x, sc.T, seed=6, first_draw=3, draws=256, **kw)
    assert not np.array_equal(a[0], c[0]) and a[1:] == c[1:]
    h1 = cake_amd.op_sample(x, sc.T, seed=5, first_draw=3, draws=128, **kw)
    h2 = cake_amd.op_sample(x, sc.T, seed=5, first_draw=131, draws=128, **kw)
    assert np.array_equal(np.concatenate([h1[0], h2[0]]), a[0])


def test_op_validation_errors():
    x = np.zeros(8, dtype=np.float32)
    bad = [
        dict(draws=0), dict(draws=8193), dict(first_draw=-1),
        dict(history=[0] * 1025), dict(history=[8]),
        dict(repeat_penalty=0.0), dict(repeat_penalty=-1.0),
        dict(repeat_penalty=float("nan")), dict(top_p=float("nan")),
    ]
    for kw in bad:
        with pytest.raises(cake_amd.CakeHipError):
            cake_amd.op_sample(x, kw.pop("temperature", 0.7), **kw)
    with pytest.raises(cake_amd.CakeHipError):
        cake_amd.op_sample(x, float("nan"))
    with pytest.raises(cake_amd.CakeHipError):
        cake_amd.op_sample(np.zeros(0, dtype=np.float32), 0.7)
    with pytest.raises(cake_amd.CakeHipError):
        cake_amd.op_sample(np.zeros((1 << 18) + 1, dtype=np.float32), 0.7)


# ---------------------------------------------------------------------------
# engine level (the tiny llama of test_gumbel_sampling_semantics)
# ---------------------------------------------------------------------------
CFG = dict(
    model_type="llama", hidden_size=128, intermediate_size=256,
    vocab_size=512, num_hidden_layers=2, num_attention_heads=4,
    num_key_value_heads=2, head_dim=32, max_position_embeddings=256)
PROMPT = np.arange(10, dtype=np.uint32)
ALL_ON = dict(top_k=20, top_p=0.9, repeat_penalty=1.3, repeat_last_n=4,
              seed=7)


def _engine(graph):
    flags = cake_amd.HAS_EMBED | cake_amd.HAS_HEAD
    if graph:
        flags |= cake_amd.USE_GRAPH
    eng = cake_amd.Engine(json.dumps(CFG), max_seq=256, max_batch_tokens=64,
                          flags=flags)
    eng.init_random(seed=3)
    return eng


@pytest.fixture(scope="module")
def eng():
    e = _engine(True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_eager():
    e = _engine(False)
    yield e
    e.close()


def _stepwise(e, n):
    """Prefill + single-token append-prefills: [(token, raw logits)]."""
    e.reset()
    out = [e.prefill(PROMPT, want_logits=True)]
    for _ in range(n - 1):
        out.append(e.prefill(np.array([out[-1][0]], dtype=np.uint32),
                             want_logits=True))
    return out


def test_engine_all_off_is_set_sampling(eng, eng_eager):
    for e in (eng, eng_eager):
        for temp in (0.8, 0.0):
            e.set_sampling(temp, seed=5)
            want = e.generate_greedy(PROMPT, 12)
            e.set_sampling_ex(temp, top_k=0, top_p=1.0, repeat_penalty=1.0,
                              repeat_last_n=128, seed=5)
            assert e.generate_greedy(PROMPT, 12) == want
            e.set_sampling_ex(temp, top_k=512, top_p=0.0, repeat_penalty=1.5,
                              repeat_last_n=0, seed=5)
            assert e.generate_greedy(PROMPT, 12) == want


def test_engine_degenerate_selection_is_greedy(eng):
    eng.set_sampling(0.0)
    steps = _stepwise(eng, 12)
    for _, lg in steps:
        top2 = np.sort(lg)[-2:]
        assert top2[0] != top2[1], "precondition: no exact top-2 tie"
    greedy = [t for t, _ in steps]
    for kw in (dict(top_k=1), dict(top_p=1e-6)):
        eng.set_sampling_ex(0.8, seed=3, **kw)
        assert [t for t, _ in _stepwise(eng, 12)] == greedy
    eng.set_sampling(0.0)


def test_engine_stepwise_membership_and_raw_logits(eng):
    eng.set_sampling_ex(0.8, **ALL_ON)
    steps = _stepwise(eng, 12)
    hist = []
    for tok, lg in steps:
        ref = sr.sample_ref(lg, 0.8, ALL_ON["top_k"],
                            ALL_ON["top_p"] + sc.MARGIN,
                            ALL_ON["repeat_penalty"], hist,
                            last_n=ALL_ON["repeat_last_n"])
        assert ref["mask"][tok], (len(hist), tok)
        hist.append(tok)
    # the same token path with every option off returns the same logits
    eng.set_sampling(0.0)
    eng.reset()
    _, lg = eng.prefill(PROMPT, want_logits=True)
    assert np.array_equal(lg, steps[0][1])
    for (tok, _), (_, want) in zip(steps[:-1], steps[1:]):
        _, lg = eng.prefill(np.array([tok], dtype=np.uint32),
                            want_logits=True)
        assert np.array_equal(lg, want)


def test_engine_greedy_penalty_stepwise(eng):
    eng.set_sampling_ex(0.0, repeat_penalty=1.5, repeat_last_n=3)
    hist = []
    for tok, lg in _stepwise(eng, 12):
        lp = sr.penalise(lg, 1.5, hist, last_n=3)
        assert tok == sr.greedy_token(lp), len(hist)
        hist.append(tok)
    eng.set_sampling(0.0)
    plain = [t for t, _ in _stepwise(eng, 12)]
    print(f"greedy with penalty {hist}\ngreedy without    {plain}")


def test_engine_graph_equals_eager(eng, eng_eager):
    seqs = []
    for e in (eng, eng_eager):
        e.set_sampling_ex(0.8, **ALL_ON)
        seqs.append(e.generate_greedy(PROMPT, 13))
        # second run of the same prompt replays the captured prefill graph
        assert e.generate_greedy(PROMPT, 13) == seqs[-1]
    assert seqs[0] == seqs[1]


def test_engine_state_carries_across_decode_calls(eng):
    eng.set_sampling_ex(0.8, **ALL_ON)
    eng.reset()
    first = eng.prefill(PROMPT)
    one = list(eng.decode(16))
    eng.reset()
    assert eng.prefill(PROMPT) == first, "reset() restores the sequence"
    two = list(eng.decode(8)) + list(eng.decode(8))
    assert two == one  # draw counter and history are not per-call state
    assert len(set(one)) > 1


def test_engine_set_sampling_restores_plain_greedy(eng):
    eng.set_sampling(0.0)
    greedy = eng.generate_greedy(PROMPT, 12)
    eng.set_sampling_ex(0.8, **ALL_ON)
    assert eng.generate_greedy(PROMPT, 12) != greedy
    eng.set_sampling(0.0)
    assert eng.generate_greedy(PROMPT, 12) == greedy


def test_engine_setter_validation(eng):
    for kw in (dict(repeat_last_n=-1), dict(repeat_last_n=1025),
               dict(repeat_penalty=0.0), dict(repeat_penalty=float("nan")),
               dict(top_p=float("nan"))):
        with pytest.raises(cake_amd.CakeHipError):
            eng.set_sampling_ex(0.8, **kw)
    with pytest.raises(cake_amd.CakeHipError):
        eng.set_sampling_ex(float("nan"))
    eng.set_sampling_ex(0.8, repeat_last_n=1024, repeat_penalty=1.1)
    eng.set_sampling(0.0)
