"""CPU tests of the gemma3 family: the committed fixture against the oracle of
tests/gemma3_ref.py (HF's logits and greedy ids, the defect and headroom
conditions of tools/gen_golden_gemma3.py), and the engine's host-only side:
the layer plan for every config spelling, the refusals, both rope tables and
weight_bytes."""
import json
import os

import numpy as np
import pytest

import cake_amd
from cake_amd.configs import GEMMA3_MODELS, find_model, weight_bytes
from tests import gemma3_ref as gr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_SEQ = 64
GPU_GATE = 2e-2


@pytest.fixture(scope="module")
def fx():
    return gr.fixture(GOLDEN)


# ---- the fixture ---------------------------------------------------------------
def test_fixture_meets_the_issue_constraints(fx):
    cfg, t, z = fx
    assert cfg["head_dim"] == 256 and cfg["num_key_value_heads"] == 1
    assert cfg["layer_types"][:3] == ["sliding_attention", "full_attention",
                                      "sliding_attention"]
    assert cfg["sliding_window"] == 8 and len(z["prompt"]) == 17
    assert len(z["hf_gen"]) == 12
    assert cfg["query_pre_attn_scalar"] != cfg["head_dim"]
    theta_g, factor_g = gr.rope_params(cfg, False)
    theta_l, factor_l = gr.rope_params(cfg, True)
    assert factor_g != 1.0 and theta_g != theta_l and factor_l == 1.0
    biggest = max(os.path.getsize(os.path.join(GOLDEN, n))
                  for n in os.listdir(GOLDEN)
                  if n.endswith(".npz") and n != "tiny_gemma3.npz")
    assert os.path.getsize(os.path.join(GOLDEN, "tiny_gemma3.npz")) <= biggest


def test_oracle_matches_hf(fx):
    cfg, t, z = fx
    o = gr.Gemma3Oracle(cfg, t, MAX_SEQ)
    lg = o.forward(z["prompt"][None, :].astype(np.int64), 0)[0]
    assert gr.rel(lg, z["hf_logits"]) < 2e-4
    ids = gr.Gemma3Oracle(cfg, t, MAX_SEQ).generate_greedy(
        list(z["prompt"]), len(z["hf_gen"]))
    assert ids == [int(x) for x in z["hf_gen"]]


def test_every_defect_shows_and_bf16_has_headroom(fx):
    cfg, t, z = fx
    moves, base = gr.defect_moves(cfg, t, z["prompt"], MAX_SEQ)
    assert set(moves) == set(gr.DEFECTS) and len(gr.DEFECTS) == 10
    for d, m in moves.items():
        print(f"{d}: logits move {m:.4f}")
        assert m >= 4 * GPU_GATE, (d, m)
    est = gr.Gemma3Oracle(cfg, t, MAX_SEQ, act_bf16=True).forward(
        z["prompt"][None, :].astype(np.int64), 0)[0]
    assert gr.rel(est, z["hf_logits"]) <= GPU_GATE / 2


# ---- the layer plan ------------------------------------------------------------
def _old_spelling(cfg):
    """The fixture's config with sliding_window_pattern, rope_theta,
    rope_local_base_freq and rope_scaling instead of layer_types and
    rope_parameters."""
    c = {k: v for k, v in cfg.items()
         if k not in ("layer_types", "rope_parameters")}
    full = cfg["rope_parameters"]["full_attention"]
    c.update(sliding_window_pattern=2, rope_theta=full["rope_theta"],
             rope_local_base_freq=cfg["rope_parameters"]["sliding_attention"][
                 "rope_theta"],
             rope_scaling=dict(rope_type=full["rope_type"],
                               factor=full["factor"]))
    return c


def _plan(cfg, layers):
    return [cake_amd.layer_dispatch(cfg, i) for i in range(layers)]


def test_layer_plan_of_the_fixture_in_both_spellings(fx):
    cfg = fx[0]
    want_q = np.float32(np.sqrt(np.float32(256.0 / 128.0)))
    want = [dict(window=8, rope_table="local", q_scale=want_q),
            dict(window=0, rope_table="global", q_scale=want_q),
            dict(window=8, rope_table="local", q_scale=want_q)]
    assert _plan(cfg, 3) == want
    old = _old_spelling(cfg)
    assert gr.layer_kinds(old) == gr.layer_kinds(cfg) == [True, False, True]
    assert _plan(old, 3) == want
    for loc in (False, True):
        a = cake_amd.rope_tables(cfg, MAX_SEQ, local=loc)
        b = cake_amd.rope_tables(old, MAX_SEQ, local=loc)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(cake_amd.CakeHipError, match="outside"):
        cake_amd.layer_dispatch(cfg, 3)


def test_layer_types_in_any_order_and_others_unchanged(fx):
    cfg = dict(fx[0], layer_types=["full_attention", "sliding_attention",
                                   "full_attention"])
    assert [p["window"] for p in _plan(cfg, 3)] == [0, 8, 0]
    # every other model type keeps the full-then-sliding condensation and its
    # refusal
    q = dict(find_model("qwen3-0.6b"), sliding_window=16, num_hidden_layers=3)
    ok = dict(q, layer_types=["full_attention", "sliding_attention",
                              "sliding_attention"])
    assert [p["window"] for p in _plan(ok, 3)] == [0, 16, 16]
    assert all(p["rope_table"] == "global" and p["q_scale"] == 1
               for p in _plan(ok, 3))
    bad = dict(q, layer_types=["sliding_attention", "full_attention",
                               "sliding_attention"])
    with pytest.raises(cake_amd.CakeHipError, match="full-then-sliding"):
        cake_amd.layer_dispatch(bad, 0)


def test_nested_gemma3_with_defaults():
    """model_type gemma3: the nested text_config, HF's Gemma3TextConfig
    defaults (checked against the installed transformers) for the rest."""
    transformers = pytest.importorskip("transformers")
    hf = transformers.Gemma3TextConfig()
    nested = dict(model_type="gemma3", text_config=dict(num_hidden_layers=12),
                  vision_config=dict(hidden_size=64))
    plan = _plan(nested, 12)
    kinds = [k == "sliding_attention" for k in hf.layer_types[:12]]
    assert kinds == [True] * 5 + [False] + [True] * 5 + [False]
    assert [p["window"] for p in plan] == \
        [hf.sliding_window if k else 0 for k in kinds]
    assert [p["rope_table"] for p in plan] == \
        ["local" if k else "global" for k in kinds]
    assert hf.query_pre_attn_scalar == hf.head_dim == 256
    assert all(p["q_scale"] == 1 for p in plan)
    assert (hf.num_attention_heads, hf.num_key_value_heads, hf.vocab_size,
            hf.rms_norm_eps, hf.hidden_size, hf.intermediate_size) == \
        (8, 4, 262208, 1e-6, 2304, 9216)
    # the defaults reach the tables: head_dim 256, thetas 1e6 and 1e4
    flat = dict(model_type="gemma3_text", num_hidden_layers=12)
    for loc, theta in ((False, hf.rope_parameters["full_attention"][
            "rope_theta"]), (True, hf.rope_parameters["sliding_attention"][
                "rope_theta"])):
        cos, _ = cake_amd.rope_tables(nested, 32, local=loc)
        assert cos.shape == (32, 128)
        want = np.cos(1.0 / np.power(theta, 2.0 * 127 / 256))
        assert abs(float(cos[1, 127]) - want) < 1e-6
        assert np.array_equal(cos, cake_amd.rope_tables(flat, 32, local=loc)[0])
    assert theta == 1e4
    # 27B: sqrt(128 / 168)
    p27 = cake_amd.layer_dispatch(find_model("gemma-3-27b"), 5)
    assert p27["rope_table"] == "global" and p27["window"] == 0
    assert p27["q_scale"] == np.float32(np.sqrt(np.float32(128.0 / 168.0)))
    assert cake_amd.layer_dispatch(find_model("gemma-3-27b"), 4)["window"] \
        == 1024


# ---- refusals (host only: parse_config runs ahead of any device call) ---------
@pytest.mark.parametrize("change,match", [
    (dict(final_logit_softcapping=30.0), "final_logit_softcapping"),
    (dict(attn_logit_softcapping=50.0), "attn_logit_softcapping"),
    (dict(hidden_activation="gelu"), "hidden_activation gelu"),
    (dict(use_bidirectional_attention=True), "use_bidirectional_attention"),
    (dict(quantization_config=dict(quant_method="fp8",
                                   weight_block_size=[128, 128])),
     "quant_method fp8 with model_type gemma3"),
    (dict(quantization_config=dict(quant_method="gptq", bits=4,
                                   group_size=128)),
     "quant_method gptq with model_type gemma3"),
])
def test_refusals(fx, change, match):
    cfg = dict(fx[0], **change)
    with pytest.raises(cake_amd.CakeHipError, match=match):
        cake_amd.layer_dispatch(cfg, 0)
    with pytest.raises(cake_amd.CakeHipError, match=match):
        cake_amd.rope_tables(cfg, MAX_SEQ)
    with pytest.raises(cake_amd.CakeHipError, match=match):   # create itself
        cake_amd.Engine(json.dumps(cfg), max_seq=MAX_SEQ,
                        max_batch_tokens=MAX_SEQ)
    nested = dict(model_type="gemma3", text_config={
        k: v for k, v in cfg.items() if k != "quantization_config"})
    if "quantization_config" in cfg:       # top level in the nested form
        nested["quantization_config"] = cfg["quantization_config"]
    with pytest.raises(cake_amd.CakeHipError, match=match):
        cake_amd.layer_dispatch(nested, 0)


def test_local_table_needs_gemma3():
    with pytest.raises(cake_amd.CakeHipError, match="only a gemma3 config"):
        cake_amd.rope_tables(find_model("qwen3-0.6b"), 64, local=True)


# ---- rope tables ---------------------------------------------------------------
@pytest.mark.parametrize("name,max_seq", [("tiny", MAX_SEQ),
                                          ("gemma-3-1b", 512),
                                          ("gemma-3-4b", 4096)])
@pytest.mark.parametrize("local", [False, True], ids=["global", "local"])
def test_rope_tables_vs_float64(fx, name, max_seq, local):
    """The bound of the LongRoPE table tests (tests/test_rotary_ref.py) with
    m = 1: 2^-22 |a| + 2^-22, a the angle.  The frequency is evaluated in
    double and rounded once, so it and the position product stay under 2^-22
    relative on a; cosf / sinf add under one ulp of a value <= 1."""
    cfg = fx[0] if name == "tiny" else find_model(name)
    cos, sin = cake_amd.rope_tables(cfg, max_seq, local=local)
    c64, s64, a = gr.rope_tables64(cfg, max_seq, local)
    assert cos.shape == sin.shape == c64.shape == (
        max_seq, gr.text_config(cfg)["head_dim"] // 2)
    bound = 2.0 ** -22 * np.abs(a) + 2.0 ** -22
    worst = max(np.max(np.abs(cos - c64) / bound),
                np.max(np.abs(sin - s64) / bound))
    print(f"{name} local={local}: engine tables at {worst:.3f} of the bound")
    assert worst <= 1.0
    c32, s32 = gr.rope_tables32(cfg, max_seq, local)
    w32 = max(np.max(np.abs(c32 - c64) / bound),
              np.max(np.abs(s32 - s64) / bound))
    assert w32 <= 1.0
    theta, factor = gr.rope_params(cfg, local)
    want = 1.0 / (factor * np.power(theta, 2.0 * np.arange(a.shape[1]) /
                                    (2 * a.shape[1])))
    assert np.allclose(a[1], want, rtol=1e-12)


def test_the_two_tables_differ_and_linear_divides(fx):
    cfg = fx[0]
    g = cake_amd.rope_tables(cfg, MAX_SEQ)[0]
    loc = cake_amd.rope_tables(cfg, MAX_SEQ, local=True)[0]
    assert not np.array_equal(g, loc)
    plain = json.loads(json.dumps(cfg))
    plain["rope_parameters"]["full_attention"] = dict(
        rope_type="default", rope_theta=1000000.0)
    p = cake_amd.rope_tables(plain, MAX_SEQ)[0]
    # factor 4: position 4 of the scaled table is position 1 of the plain one
    assert np.max(np.abs(g[4] - p[1])) < 2.0 ** -21
    assert not np.allclose(g[4], p[4])


# ---- configs ---------------------------------------------------------------------
def test_models_and_weight_bytes(fx):
    assert set(GEMMA3_MODELS) == {"gemma-3-1b", "gemma-3-4b", "gemma-3-12b",
                                  "gemma-3-27b"}
    for name, cfg in GEMMA3_MODELS.items():
        assert find_model(name) is cfg
        cake_amd.layer_dispatch(cfg, cfg["num_hidden_layers"] - 1)
    cfg, t, _ = fx
    assert weight_bytes(cfg) == 2 * sum(v.size for v in t.values())
    H, hd = cfg["hidden_size"], cfg["head_dim"]
    one = weight_bytes(cfg, 1, 2, embed=False, head=False)
    names = [k for k in t if k.startswith("model.layers.1.")]
    assert one == 2 * sum(t[k].size for k in names)
    assert sum(k.endswith("norm.weight") for k in names) == 6
    assert weight_bytes(cfg, embed=False) - 3 * one == 2 * H   # model.norm
    # the same model as a llama counts two norm rows and no q/k rows
    llama = dict(cfg, model_type="llama")
    assert weight_bytes(cfg) - weight_bytes(llama) == 3 * 2 * (2 * H + 2 * hd)
