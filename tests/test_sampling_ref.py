"""CPU tests of the sampler reference and its case generator: the conditions
the GPU tests rely on (margins, distinct top-k boundaries, the chi-square
bound on the reference stream) and the reference's sensitivity to each of
the defects it is meant to catch."""
import numpy as np
import pytest

from tests import sampling_cases as sc
from tests import sampling_ref as sr

SMALL_VS = tuple(v for v in sc.VS if v <= 4099)
CHI_SEEDS = (1, 2, 3, 299792458)
CHI_VS = (1000, 4099)
CHI_BOUND = 31.0  # the 1e-6 tail of chi-square at 3 degrees of freedom


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_margin_and_distinct_boundaries(family):
    """Every generated top-p value sits >= 2^-10 of renormalised mass away
    from the cumulative mass on both sides of its boundary token; every
    top-k boundary separates two different values."""
    n_p = 0
    for V in sc.VS:
        for i, c in enumerate(sc.cases(family, V)):
            ref = sc.reference(family, V, i)
            if c["mode"] in ("p", "kp"):
                n_p += 1
                assert ref["before"] <= c["top_p"] - sc.MARGIN, (V, c["name"])
                assert ref["upto"] >= c["top_p"] + sc.MARGIN, (V, c["name"])
                assert ref["kept"] >= 1
            if c["mode"] == "k" and 0 < c["top_k"] < V and family != "equal":
                s = np.sort(ref["lp"])[::-1]
                if family == "neginf" and np.isneginf(s[c["top_k"] - 1]):
                    # deliberate tie: k reaches into the -inf group, which
                    # is the bottom of the order and survives whole
                    assert ref["kept"] == V, (V, c["name"])
                    continue
                assert s[c["top_k"] - 1] != s[c["top_k"]], (V, c["name"])
                assert ref["kept"] == c["top_k"]
            assert ref["kept"] == int(np.sum(ref["lp"] >= ref["tau"]))
    assert n_p >= (2 if family == "equal" else 20)


def test_case_coverage():
    """The generator produces what the GPU test is asked to cover."""
    names = {c["name"] for f in sc.FAMILIES for V in sc.VS
             for c in sc.cases(f, V)}
    for want in ("k1", "k2", "k40", "k40+pen", "p@0", "p@199", "p@100+pen",
                 "k40p@20", "k40p@39+pen", "k3p@1"):
        assert want in names, want
    assert np.isneginf(sc.make_logits("neginf", 1000)[0]).sum() == 5
    assert np.abs(sc.make_logits("big", 1000)[0]).max() == 1e4
    assert 0.0 in sc.make_logits("mixed", 1000)[0]
    assert (sc.make_logits("negative", 4099)[0] < 0).all()


def _moved(mut, mode, penalised=False):
    for family in sc.FAMILIES:
        for V in SMALL_VS:
            for i, c in enumerate(sc.cases(family, V)):
                if c["mode"] != mode or (penalised and c["penalty"] == 1.0):
                    continue
                a = sc.reference(family, V, i)
                b = sc.reference(family, V, i, mut)
                if a["kept"] != b["kept"] or a["tau"] != b["tau"]:
                    return True
    return False


@pytest.mark.parametrize("mut,mode,penalised", [
    ("k_minus", "k", False), ("k_minus", "kp", False),
    ("k_plus", "k", False), ("k_plus", "kp", False),
    ("prefix_short", "p", False), ("prefix_short", "kp", False),
    ("prefix_long", "p", False), ("prefix_long", "kp", False),
    ("renorm_all", "kp", False),
    ("sign_blind", "k", True), ("sign_blind", "p", True),
    ("sign_blind", "kp", True),
    ("dup_twice", "k", True), ("dup_twice", "p", True),
    ("dup_twice", "kp", True),
    ("bad_key", "k", False), ("bad_key", "p", False),
    ("bad_key", "kp", False),
])
def test_sensitivity(mut, mode, penalised):
    """Each defect moves `kept` or tau on at least one case of every case
    family (top-k / top-p / k-then-p, with penalty where the defect is in
    the penalty) it can affect."""
    assert mut in sr.MUTATIONS
    assert _moved(mut, mode, penalised)


@pytest.mark.parametrize("family", [f for f in sc.FAMILIES if f != "equal"])
def test_sensitivity_per_logit_family(family):
    """Off-by-one in k and a prefix off by one show in every logit family
    except the all-equal one, where the tie rule keeps everything."""
    for mut in ("k_minus", "prefix_long"):
        hit = False
        for V in SMALL_VS:
            for i, c in enumerate(sc.cases(family, V)):
                a = sc.reference(family, V, i)
                b = sc.reference(family, V, i, mut)
                hit |= a["kept"] != b["kept"] or a["tau"] != b["tau"]
        assert hit, mut


def test_tie_rule():
    x, k, kept, tau = sc.tie_case(1000)
    ref = sr.select(x, sc.T, top_k=k)
    assert ref["kept"] == kept and ref["tau"] == tau
    eq = np.full(255, -3.25, dtype=np.float32)
    for kw in (dict(top_k=7), dict(top_p=0.5), dict(top_k=7, top_p=0.5)):
        ref = sr.select(eq, sc.T, **kw)
        assert ref["kept"] == 255 and ref["tau"] == np.float32(-3.25)


def test_penalty_rule():
    x = np.array([2.0, -2.0, 0.0, -0.0, 5.0], dtype=np.float32)
    lp = sr.penalise(x, 1.1, [0, 1, 2, 3, 0, 1])
    inv = np.float32(1.0) / np.float32(1.1)
    assert lp[0] == np.float32(2.0) * inv
    assert lp[1] == np.float32(-2.0) * np.float32(1.1)
    assert lp[2] == 0 and lp[3] == 0 and lp[4] == 5
    assert np.array_equal(sr.penalise(x, 1.1, [4, 0, 1], last_n=2),
                          sr.penalise(x, 1.1, [0, 1]))
    assert np.array_equal(sr.penalise(x, 1.1, [0], last_n=0), x)
    assert np.array_equal(sr.penalise(x, 1.0, [0]), x)


def test_keys_order():
    x = np.array([-np.inf, -1e4, -1.5, -1e-30, 0.0, 1e-30, 2.0, 1e4],
                 dtype=np.float32)
    k = sr.keys(x).astype(np.int64)
    assert (np.diff(k) > 0).all()
    assert sr.keys(np.float32(-0.0)) == sr.keys(np.float32(0.0))
    assert not (np.diff(sr.keys(x, "bad_key").astype(np.int64)) > 0).all()


def test_uniform_stream_restatement():
    """Spot values of the splitmix64 stream worked by hand in Python ints,
    and uniform_at == uniform_stream on a subset."""
    M = (1 << 64) - 1
    seed, draw, i = 299792458, 5, 17

    def u_of(seed, draw, i):
        z = (seed + 0x9e3779b97f4a7c15 * (draw + 1) +
             0xbf58476d1ce4e5b9 * (i + 1)) & M
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M
        z ^= z >> 31
        # the contract, in integers: (min(k, 2^24 - 2) + 1) / 2^24
        return (min(z >> 40, (1 << 24) - 2) + 1) / (1 << 24)

    u = sr.uniform_stream(seed, draw, 64)
    assert u[i] == u_of(seed, draw, i)
    assert (u > 0).all() and (u < 1).all()
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    sub = sr.uniform_at(seed, [draw, draw + 1], [3, i])
    assert sub[0, 1] == u[i] and sub[0, 0] == u[3]
    assert sub[1, 0] == u_of(seed, draw + 1, 3)


def test_uniform_stream_stays_inside_the_open_interval_at_the_extremes():
    """The hash bits k = 2^24 - 1 (where the f32 expression ((float)k + 1) *
    (1 / 16777217.0f) gave exactly 1, hence +inf noise) and k = 0."""
    from tests import head_cases as hc
    for k, (seed, draw, i) in hc.extreme_rows():
        u = sr.uniform_stream(seed, draw, hc.EXTREMES_V)
        assert (u > 0).all() and (u < 1).all()
        assert u[i] == u_of_k(k) == sr.uniform_at(seed, [draw], [i])[0, 0]
        assert np.isfinite(sr.gumbel(seed, draw, hc.EXTREMES_V)).all()
    seed, draw, i = hc.POISON_PRODUCT
    u = sr.uniform_stream(seed, draw, hc.PRODUCT_V)
    assert u[i] == 1 - 2.0 ** -24 and u.max() == u[i] and u.min() > 0


def u_of_k(k):
    return (min(k, (1 << 24) - 2) + 1) / (1 << 24)


def test_op_sample_validates_before_any_device_call():
    """Error 5 comes back on a machine without a GPU."""
    import cake_amd
    x = np.zeros(8, dtype=np.float32)
    for kw in (dict(draws=0), dict(draws=8193), dict(first_draw=-1),
               dict(history=[0] * 1025), dict(history=[8]),
               dict(repeat_penalty=0.0), dict(repeat_penalty=float("nan")),
               dict(top_p=float("nan"))):
        with pytest.raises(cake_amd.CakeHipError):
            cake_amd.op_sample(x, 0.7, **kw)
    for bad in (np.zeros(0, dtype=np.float32),
                np.zeros((1 << 18) + 1, dtype=np.float32)):
        with pytest.raises(cake_amd.CakeHipError):
            cake_amd.op_sample(bad, 0.7)


@pytest.mark.parametrize("V", CHI_VS)
@pytest.mark.parametrize("seed", CHI_SEEDS)
def test_chi_square_of_reference_stream(V, seed):
    """4096 consecutive reference draws on the .4/.3/.2/.1 support stay
    under the bound the GPU test asserts for the device."""
    x, ids, probs = sc.chi_case(V)
    ref = sr.select(x, sc.T, top_k=4)
    assert ref["kept"] == 4 and set(np.flatnonzero(ref["mask"])) == set(ids)
    toks = sr.draws_on_support(x, ids, sc.T, seed, 0, 4096)
    assert sr.chi_square(toks, ids, probs) < CHI_BOUND
    # the subset shortcut is the full draw
    for d in (0, 7):
        assert toks[d] == sr.draw_ref(x, ref["mask"], sc.T, seed, d)
