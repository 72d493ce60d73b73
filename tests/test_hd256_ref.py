"""CPU half of the head_dim-256 tests: the geometry rule and the host-side
routing queries, the Falcon3 configs' dispatch, the teeth condition of
tests/test_attn_ref.py on every hd-256 shape tests/test_hd256_ops_gpu.py runs
(a shape that fails gets other inputs, never another threshold), and the
committed fixture tests/golden/tiny_falcon3."""
import json
import os

import numpy as np
import pytest

import cake_amd
from cake_amd.configs import FALCON3_MODELS, MODELS, find_model
from tests import attn_cases as ac
from tests import falcon3_ref as fr
from tests import hd256_cases as hc
from tests import linear_cases as lc
from tests import rotary_cases as rc
from tests import test_attn_ref as tar
from tests import test_linear_ref as tlr
from tests import test_rotary_ref as trr
from tests.helpers import fixture_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = cake_amd.CakeHipError


@pytest.fixture(autouse=True)
def _no_knob(monkeypatch):
    monkeypatch.delenv("CAKE_ATTN256_GB", raising=False)


# ---- geometry rule -------------------------------------------------------------
def _attn_args(hd, nh=4, nkv=2, max_seq=64, S=3):
    q = np.zeros((S, nh, hd), np.float32)
    kc = np.zeros((nkv, max_seq, hd), np.float32)
    return q, kc, np.zeros((nkv, hd, max_seq), np.float32)


@pytest.mark.parametrize("hd", [136, 192, 264])
def test_other_wide_heads_stay_refused_and_named(hd):
    q, kc, vtc = _attn_args(hd)
    with pytest.raises(E, match=f"op_attn_prefill.*hd {hd}"):
        cake_amd.op_attn_prefill(q, kc, kc, vtc, 0)
    with pytest.raises(E, match=f"op_attn_decode.*hd {hd}"):
        cake_amd.op_attn_decode(q[0], kc, kc, 0)
    with pytest.raises(E, match=f"head_dim {hd}"):
        cake_amd.Engine(_cfg(hd), max_seq=32)


def test_hd_256_passes_the_argument_checks():
    """The checks run in order and ahead of any device call: with hd 256 each
    entry now reaches the check BEHIND the geometry rule."""
    q, kc, vtc = _attn_args(256)
    with pytest.raises(E, match="op_attn_decode: pos 64 outside the cache"):
        cake_amd.op_attn_decode(q[0], kc, kc, 64)
    with pytest.raises(E, match="op_attn_prefill: rows .* outside the cache"):
        cake_amd.op_attn_prefill(q, kc, kc, vtc, 62)
    # the variants: the MFMA-256 kernel and the plain one, nothing of hd 128's
    for bad in ((2, 8, 0, 0), (2, 4, 0, 0), (1, 8, 0, 0), (1, 4, 1, 0),
                (0, 4, 0, 0)):
        with pytest.raises(E, match="not dispatchable at hd 256"):
            cake_amd.op_attn_prefill(q, kc, kc, vtc, 0, 0, bad)
    # and hd 128 does not take hd 256's
    q, kc, vtc = _attn_args(128)
    with pytest.raises(E, match="not dispatchable at hd 128"):
        cake_amd.op_attn_prefill(q, kc, kc, vtc, 0, 0, hc.PF_MFMA)


def _cfg(hd, **kw):
    return dict(dict(
        model_type="llama", hidden_size=64, intermediate_size=128,
        vocab_size=128, num_hidden_layers=1, num_attention_heads=2,
        num_key_value_heads=1, head_dim=hd), **kw)


def test_engine_create_accepts_hd_256():
    """Without a GPU the create fails at the first device call; with one it
    succeeds.  Either way the geometry rule lets head_dim 256 through."""
    try:
        eng = cake_amd.Engine(_cfg(256), max_seq=32)
    except E as e:
        assert "head_dim" not in str(e), e
        assert "hip error" in str(e), e
    else:
        eng.close()


# ---- routing queries (host only) -------------------------------------------------
def test_decode_path_and_group():
    for nchunk in (1, 4, 8, 64):
        for nh, nkv in hc.DEC_GEOM + ((12, 4),):
            assert cake_amd.attn_decode_path(nh, nkv, 256, nchunk) == 3
    # the default is the per-head route: grouping measured slower
    for G in (2, 3, 4, 5, 6, 8):
        assert cake_amd.attn_decode_group(G, 1, 256) == 1
        assert cake_amd.attn_dispatch(1, G, 1, 256)["decode_grid_y"] == G
    # hd <= 128 answers what it did
    assert cake_amd.attn_decode_path(32, 8, 128, 16) == 1
    assert cake_amd.attn_decode_path(6, 2, 128, 8) == 0
    assert cake_amd.attn_decode_group(32, 8, 128) == 4
    assert cake_amd.attn_decode_group(6, 2, 128) == 1
    assert cake_amd.attn_decode_group(4, 2, 64) == 1


def test_group_under_the_knob(monkeypatch):
    # cap 4: the largest of 4, 3, 2, 1 that divides G
    monkeypatch.setenv("CAKE_ATTN256_GB", "4")
    got = [cake_amd.attn_decode_group(g, 1, 256) for g in (2, 3, 4, 5, 6, 8)]
    assert got == [2, 3, 4, 1, 3, 4]
    for G, gb in hc.GROUP_OF_G.items():
        assert cake_amd.attn_decode_group(2 * G, 2, 256) == gb
        d = cake_amd.attn_dispatch(1, 2 * G, 2, 256)
        assert d["decode_grid_y"] == 2 * G // gb       # nkv * G / GB
    monkeypatch.setenv("CAKE_ATTN256_GB", "1")
    for G in (2, 3, 4, 5, 6, 8):
        assert cake_amd.attn_decode_group(G, 1, 256) == 1
        assert cake_amd.attn_dispatch(1, G, 1, 256)["decode_grid_y"] == G
    monkeypatch.setenv("CAKE_ATTN256_GB", "2")
    got = [cake_amd.attn_decode_group(G, 1, 256) for G in (2, 3, 4, 6, 8)]
    assert got == [2, 1, 2, 2, 2]
    monkeypatch.setenv("CAKE_ATTN256_GB", "3")
    assert cake_amd.attn_decode_group(12, 4, 256) == 3
    assert cake_amd.attn_decode_group(8, 1, 256) == 2
    # hd 128 does not read it
    assert cake_amd.attn_decode_group(32, 8, 128) == 4


def test_prefill_policy_at_hd_256():
    for S in (1, 17, 2048):
        d = cake_amd.attn_dispatch(S, 12, 4, 256)
        assert (d["pfv"], d["nw"], d["split"], d["deep"]) == hc.PF_MFMA


# ---- configs -----------------------------------------------------------------
def test_falcon3_configs():
    assert set(FALCON3_MODELS) == {"falcon3-1b", "falcon3-3b", "falcon3-7b",
                                   "falcon3-10b"}
    assert not set(FALCON3_MODELS) & set(MODELS)
    shape = {"falcon3-1b": (2048, 8192, 18, 8),
             "falcon3-3b": (3072, 9216, 22, 12),
             "falcon3-7b": (3072, 23040, 28, 12),
             "falcon3-10b": (3072, 23040, 40, 12)}
    for name, c in FALCON3_MODELS.items():
        assert find_model(name) is c
        assert (c["hidden_size"], c["intermediate_size"],
                c["num_hidden_layers"], c["num_attention_heads"]) == shape[name]
        assert c["model_type"] == "llama" and c["head_dim"] == 256
        assert c["num_key_value_heads"] == 4 and c["vocab_size"] == 131072
        assert c["rms_norm_eps"] == 1e-6 and c["rope_theta"] == 1000042
        assert c["tie_word_embeddings"] is False
        json.dumps(c)


def test_falcon3_decode_dispatch_is_covered_by_the_gpu_cases():
    covered = tlr._covered()
    d = cake_amd.linear_dispatch
    for K in hc.NEW_GEMV_K:          # the plain GEMV at the new K, rows 4
        x = d("plain", 64, K)
        covered.add((x["family"], 4, x["kb"]))
    x = d("gateup", 64, hc.NEW_GEMV_K[0])
    covered.add(("gateup", 4, x["kb"]))
    for name, cfg in FALCON3_MODELS.items():
        got = cake_amd.decode_dispatch(cfg)
        assert got["qkv"][0] == "qkv_rope", name     # the fused bf16 kernel
        missing = {k: v for k, v in got.items() if v not in covered}
        assert not missing, f"{name}: no GPU case runs {missing}"


# ---- case lists ----------------------------------------------------------------
def test_case_lists_are_the_issues():
    assert len(hc.DEC_CASES) == 175
    for cfg in {c[:3] for c in hc.DEC_CASES}:
        mine = [c for c in hc.DEC_CASES if c[:3] == cfg]
        assert {c[3] for c in mine} == set(ac.DEC_N), cfg
        assert {c[4] for c in mine} == set(hc.DEC_NCHUNKS), cfg
        assert {c[5] for c in mine} == set(ac.DEC_WINDOWS), cfg
        assert set(hc.DEC_SPECIALS) <= {c[3:] for c in mine}
    assert {c[:2] for c in hc.DEC_CASES} == set(hc.DEC_GEOM)
    # the specials are those of the hd-128 grouped list
    g128 = {c[3:] for c in ac.DEC_G_CASES if c[:3] == (4, 1, 128)}
    assert set(hc.DEC_SPECIALS) <= g128
    pf = hc.PF_CASES
    assert len(pf) == len(ac.PF_MFMA_ALL) + len(ac.PF_MFMA_EXTRA) + 3
    assert (4, 2, 1, 45, 0, 64) not in pf and (4, 2, 1, 65, 0, 96) in pf
    assert all(c[3] + c[2] <= c[5] and c[5] % 32 == 0 for c in pf)
    assert any(c[3] + c[2] == c[5] for c in pf)       # ends the cache
    assert {c[2] % 32 for c in pf} > {0}              # ragged S
    assert {K for *_, K, _ in hc.rope_cases()} == set(lc.ROPE_K)


# ---- teeth ---------------------------------------------------------------------
def _shapes():
    out = []
    for nh, nkv, S, pos0, w, ms in hc.PF_CASES:
        out.append((ac.TOL_MFMA, nh, nkv, hc.HD, S, pos0, w, ms, False))
    for nh, nkv, hd, n, _, w in hc.DEC_CASES:
        out.append((ac.TOL_F32P, nh, nkv, hd, 1, n - 1, w,
                    ac.decode_max_seq(n), True))
    return sorted(set(out))


@pytest.mark.parametrize("shape", _shapes(), ids=tar._shape_id)
def test_gpu_case_inputs_have_teeth(shape):
    tar.test_gpu_case_inputs_have_teeth(shape)


def test_the_swapped_prefill_shape_had_no_teeth():
    with pytest.raises(AssertionError, match="mult64_dropped"):
        tar.test_gpu_case_inputs_have_teeth(
            (ac.TOL_MFMA, 4, 2, hc.HD, 1, 45, 0, 64, False))


@pytest.mark.parametrize("case", hc.rope_cases(),
                         ids=lambda c: "-".join(map(str, c)))
def test_qkv_rope_teeth_256(case):
    tlr.test_qkv_rope_teeth(case)


@pytest.mark.parametrize("case", [
    (2, 1, 256, 128, 5, 7, False), (12, 4, 256, 128, 33, 0, False),
    (2, 1, 256, 192, 1, 45, True), (12, 4, 256, 128, 1, 63, True)],
    ids=lambda c: "-".join(map(str, c)))
def test_store_teeth_256(case):
    assert case[4] + case[5] <= rc.STORE_MAX_SEQ
    trr.test_store_teeth(case)


# ---- the committed fixture -------------------------------------------------------
GATE = 2e-2


@pytest.fixture(scope="module")
def fx():
    return fixture_weights(GOLDEN, "tiny_falcon3")


def test_fixture_is_the_issues_shape(fx):
    cfg_json, cfg, w, z = fx
    assert cfg_json["model_type"] == "llama" and cfg.hd == 256
    assert (cfg.num_attention_heads, cfg.num_key_value_heads) == (2, 1)
    assert cfg.hidden_size == 64 and cfg.num_hidden_layers == 2
    assert len(z["prompt"]) == 17 and len(z["hf_gen"]) == 12
    for k in z.files:                # every weight is a bf16 value
        if k.startswith("w."):
            a = np.ascontiguousarray(z[k], dtype=np.float32)
            assert not (a.view(np.uint32) & 0xFFFF).any(), k
    size = os.path.getsize(os.path.join(GOLDEN, "tiny_falcon3.npz"))
    others = [os.path.getsize(os.path.join(GOLDEN, n))
              for n in os.listdir(GOLDEN)
              if n.endswith(".npz") and n != "tiny_falcon3.npz"]
    assert size <= max(others)


def test_reference_matches_hf_on_the_fixture(fx):
    cfg_json, cfg, w, z = fx
    o = fr.Hd256Oracle(cfg, w, cfg_json, 64)
    lg = o.forward(z["prompt"][None, :].astype(np.int64), 0)[0]
    assert fr.rel(lg, z["hf_logits"]) < 2e-4
    o = fr.Hd256Oracle(cfg, w, cfg_json, 64)
    ids = o.generate_greedy(list(z["prompt"]), 12)
    assert ids == [int(t) for t in z["hf_gen"]]


def test_each_attention_defect_moves_the_logits(fx):
    cfg_json, cfg, w, z = fx
    moves, _ = fr.defect_moves(cfg, w, cfg_json, z["prompt"], 64)
    print("tiny_falcon3 defect moves:", moves)
    assert set(moves) == set(fr.ATTN_DEFECTS)
    for d, m in moves.items():
        assert m >= 4 * GATE, (d, m)


def test_bf16_activations_leave_headroom(fx):
    cfg_json, cfg, w, z = fx
    est = fr.Hd256Oracle(cfg, w, cfg_json, 64, act_bf16=True).forward(
        z["prompt"][None, :].astype(np.int64), 0)[0]
    assert fr.rel(est, z["hf_logits"]) <= GATE / 2
