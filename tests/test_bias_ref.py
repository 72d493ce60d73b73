"""CPU tests of the qwen2 q|k|v bias: the committed fixture and its reference,
the teeth of the GPU op tests (tests/test_bias_ops_gpu.py), and the host-only
surface (config refusals, kernel dispatch of the new configs, byte counts).

Teeth: for every call the GPU module makes, every defect of MUTANTS that fits
the shape must move some element of the reference by more than TWICE what the
GPU test grants there (any bit of V where V is held bit-exact), in at least
one of the call's input families."""
import ctypes
import json
import os

import numpy as np
import pytest

import cake_amd
from cake_amd.configs import (MODELS, QUANT_MODELS, QWEN2_MODELS, find_model,
                              weight_bytes, weight_bytes_bf16)
from tests import bias_cases as bc
from tests import qwen2_ref as qr
from tests.helpers import fixture_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GPU_GATE = 2e-2                  # relative logits limit of the engine tests
_id = lambda c: "-".join(map(str, c))


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- fixture ----------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    cfg_json, cfg, w, z = fixture_weights(GOLDEN, "tiny_qwen2")
    biases = qr.fused_biases({k[2:]: z[k] for k in z.files}, cfg)
    return cfg_json, cfg, w, z, biases


def test_fixture_is_the_issues_shape(fx):
    cfg_json, cfg, w, z, biases = fx
    assert cfg_json["model_type"] == "qwen2"
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size,
            cfg.num_hidden_layers, cfg.num_attention_heads,
            cfg.num_key_value_heads, cfg.hd) == (64, 128, 256, 2, 4, 2, 16)
    assert cfg.tie_word_embeddings and cfg.rms_norm_eps == 1e-6
    assert cfg.rope_theta == 1e6 and not cfg.use_qk_norm
    assert all(b.shape == (128,) and np.abs(b).max() > 1 for b in biases)


def test_reference_matches_hf_on_the_fixture(fx):
    cfg_json, cfg, w, z, biases = fx
    o = qr.Qwen2Oracle(cfg, w, biases)
    lg = o.forward(z["prompt"][None, :], 0)[0]
    assert _rel(lg, z["hf_logits"]) < 2e-4
    assert np.array_equal(lg, z["oracle_logits"])
    o.reset()
    gen = o.generate_greedy(list(z["prompt"]), len(z["hf_gen"]))
    assert gen == [int(t) for t in z["hf_gen"]]


@pytest.mark.parametrize("which", ["q", "k", "v"])
def test_dropping_one_bias_moves_the_logits(fx, which):
    """Condition of the fixture: an engine that drops any one of the three
    biases misses the GPU gate by a factor of four at the least."""
    cfg_json, cfg, w, z, biases = fx
    o = qr.Qwen2Oracle(cfg, w, qr.drop_one(biases, cfg, which))
    move = _rel(o.forward(z["prompt"][None, :], 0)[0], z["oracle_logits"])
    assert move >= 4 * GPU_GATE, (which, move)


def test_without_any_bias_the_logits_are_elsewhere(fx):
    """What the engine computed before it knew the family."""
    cfg_json, cfg, w, z, biases = fx
    o = qr.Qwen2Oracle(cfg, w, [0 * b for b in biases])
    assert _rel(o.forward(z["prompt"][None, :], 0)[0],
                z["oracle_logits"]) > 0.5


# ---- teeth: store kernels -----------------------------------------------------
@pytest.mark.parametrize("case", bc.store_cases(), ids=_id)
def test_store_teeth(case):
    nh, nkv, hd, S, pos0, decode = case
    fits = set()
    moved = set()
    for fam in bc.STORE_FAMILIES:
        d = bc.store_inputs(fam, *case)
        assert bc.store_sums_exact(d), "raw + b must be exact in f32"
        b = np.abs(d["bias"])
        assert b.min() >= 2.0 ** -6 and b.max() <= 2.0 ** 7
        base = bc.store_ref(d, nh, nkv, hd, pos0)
        for mut in bc.MUTANTS:
            m = bc.store_ref(d, nh, nkv, hd, pos0, mut)
            if m is None:
                continue
            fits.add(mut)
            if bc.store_moved(base, m, pos0, S):
                moved.add(mut)
    assert fits - moved == set()
    assert len(fits) >= len(bc.MUTANTS) - (1 if nkv < 2 else 0)


# ---- teeth: fused kernel ------------------------------------------------------
@pytest.mark.parametrize("case", bc.fused_cases(), ids=_id)
def test_fused_teeth(case):
    nh, nkv, hd, K, pos = case
    fits = set()
    moved = set()
    for fam in bc.FUSED_FAMILIES:
        d = bc.fused_inputs(fam, *case)
        if d["exact"]:
            assert bc.fused_sums_exact(d, nh, nkv, hd, pos)
        base = bc.fused_ref(d, nh, nkv, hd, pos)
        for mut in bc.MUTANTS:
            m = bc.fused_ref(d, nh, nkv, hd, pos, mut)
            if m is None:
                continue
            fits.add(mut)
            if bc.fused_moved(base, m, d["exact"]):
                moved.add(mut)
    assert fits - moved == set()
    assert len(fits) >= len(bc.MUTANTS) - (1 if nkv < 2 else 0)


def test_fused_cases_cover_every_kb_and_the_qwen2_shapes():
    cases = bc.fused_cases()
    kbs = {cake_amd.linear_dispatch("qkv_rope", 128, c[3])["kb"]
           for c in cases}
    assert kbs == {1, 2, 4, 8}
    assert {(7, 1, 128, 896), (7, 1, 128, 3584), (14, 2, 64, 896),
            (14, 2, 64, 3584)} <= {c[:4] for c in cases}


# ---- host-only surface --------------------------------------------------------
# recorded from the policy functions (gemv_*_kb, *_rows_policy) as they stood
# before the family was added: the bias changes no kernel choice
PINNED = {
    "qwen2.5-0.5b": dict(qkv=("qkv_rope", 4, 1), o=("gemv_reg", 2, 2),
                         gateup=("gateup", 4, 2), down=("gemv_reg", 2, 4),
                         head=("gemv_reg", 8, 2)),
    "qwen2.5-7b": dict(qkv=("qkv_rope", 4, 2), o=("gemv_reg", 2, 2),
                       gateup=("gateup", 4, 2), down=("gemv_stream", 4, 0),
                       head=("gemv_reg", 8, 2)),
    "qwen2.5-7b-gptq": dict(qkv=("gemv_w4", 4, 1), o=("gemv_w4", 4, 1),
                            gateup=("gateup_w4", 4, 1),
                            down=("gemv_w4", 4, 8), head=("gemv_reg", 8, 2)),
}


def test_decode_dispatch_of_the_new_configs():
    assert set(PINNED) == set(QWEN2_MODELS)
    for name, cfg in QWEN2_MODELS.items():
        assert cake_amd.decode_dispatch(cfg) == PINNED[name], name
        # ... and equals the per-layer policy queries on the same shapes
        H, I = cfg["hidden_size"], cfg["intermediate_size"]
        Sq = cfg["num_attention_heads"] * cfg["head_dim"]
        Nq = Sq + 2 * cfg["num_key_value_heads"] * cfg["head_dim"]
        t = lambda d: (d["family"], d["rows"], d["kb"])
        if "quantization_config" in cfg:
            q = cake_amd.linear_dispatch_w4
            want = dict(qkv=t(q("plain", Nq, H)), o=t(q("plain", H, Sq)),
                        gateup=t(q("gateup", I, H)), down=t(q("plain", H, I)))
        else:
            q = cake_amd.linear_dispatch
            want = dict(qkv=t(q("qkv_rope", Nq, H)), o=t(q("plain", H, Sq)),
                        gateup=t(q("gateup", I, H)), down=t(q("plain", H, I)))
        want["head"] = t(cake_amd.linear_dispatch("plain", cfg["vocab_size"],
                                                  H))
        assert PINNED[name] == want, name


def _create_code(cfg):
    h = ctypes.c_void_p()
    return cake_amd._lib.cake_hip_engine_create(
        json.dumps(cfg).encode(), 0, 1, 0, 64, 32, 0, ctypes.byref(h))


@pytest.mark.parametrize("model_type", ["llama", "mistral", "qwen3"])
@pytest.mark.parametrize("key", ["attention_bias", "mlp_bias"])
def test_unsupported_bias_configs_are_refused(model_type, key):
    cfg = dict(QWEN2_MODELS["qwen2.5-0.5b"], model_type=model_type)
    cfg[key] = True
    assert _create_code(cfg) == 5
    assert key in cake_amd._lib.cake_hip_last_error().decode()
    with pytest.raises(cake_amd.CakeHipError, match=key):
        cake_amd.decode_dispatch(cfg)
    cfg[key] = False                     # what HF writes for these families
    cake_amd.decode_dispatch(cfg)


def test_qwen2_config_rules():
    cfg = dict(QWEN2_MODELS["qwen2.5-0.5b"], attention_bias=True)
    assert cake_amd.decode_dispatch(cfg) == PINNED["qwen2.5-0.5b"]
    # exactly "qwen2" carries the bias: qwen2_moe and friends are other types
    other = dict(cfg, model_type="qwen2_moe")
    assert _create_code(other) == 5


def test_tables_and_byte_counts():
    assert not set(QWEN2_MODELS) & (set(MODELS) | set(QUANT_MODELS))
    for name, cfg in QWEN2_MODELS.items():
        assert find_model(name) is cfg
    assert find_model("llama3-8b") is MODELS["llama3-8b"]
    assert find_model("llama3-8b-gptq") is QUANT_MODELS["llama3-8b-gptq"]
    with pytest.raises(KeyError):
        find_model("qwen2.5-72b")
    c = QWEN2_MODELS["qwen2.5-0.5b"]
    assert (c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"],
            c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"],
            c["vocab_size"], c["tie_word_embeddings"], c["rms_norm_eps"],
            c["rope_theta"]) == (896, 4864, 24, 14, 2, 64, 151936, True,
                                 1e-6, 1e6)
    c7 = QWEN2_MODELS["qwen2.5-7b"]
    assert (c7["hidden_size"], c7["intermediate_size"],
            c7["num_hidden_layers"], c7["num_attention_heads"],
            c7["num_key_value_heads"], c7["head_dim"], c7["vocab_size"],
            c7["tie_word_embeddings"]) == (3584, 18944, 28, 28, 4, 128,
                                           152064, False)
    q = QWEN2_MODELS["qwen2.5-7b-gptq"]["quantization_config"]
    assert (q["quant_method"], q["bits"], q["group_size"],
            q["desc_act"]) == ("gptq", 4, 128, False)
    # the fused f32 bias row: L * Nq * 4 on top, in both formats
    for cfg, L, Nq in ((c, 24, 1152), (c7, 28, 4608)):
        assert weight_bytes(cfg) == weight_bytes_bf16(cfg) + L * Nq * 4
    g = QWEN2_MODELS["qwen2.5-7b-gptq"]
    assert weight_bytes(g) - weight_bytes(dict(g, model_type="llama")) == \
        28 * 4608 * 4
    assert weight_bytes(MODELS["llama3-8b"]) == \
        weight_bytes_bf16(MODELS["llama3-8b"])


def test_op_entries_validate_before_any_device_call():
    z = np.zeros
    nh, nkv, hd, ms = 2, 1, 64, 64
    Nq = (nh + 2 * nkv) * hd
    tab = z((ms, hd // 2), np.float32)
    kc, vt = z((nkv, ms, hd), np.float32), z((nkv, hd, ms), np.float32)
    E = cake_amd.CakeHipError
    with pytest.raises(E, match="outside the cache"):
        cake_amd.op_kv_store_bias(z((1, Nq)), z(Nq), tab, tab, kc, kc, vt, ms,
                                  nh, nkv)
    with pytest.raises(E, match="QK-norm"):
        cake_amd.op_kv_store_bias(z((1, Nq)), z(Nq), tab, tab, kc, kc, vt, 0,
                                  nh, nkv, q_norm=z(hd), k_norm=z(hd))
    with pytest.raises(ValueError, match="bias"):
        cake_amd.op_kv_store_bias(z((1, Nq)), z(Nq - 1), tab, tab, kc, kc, vt,
                                  0, nh, nkv)
    with pytest.raises(E, match="pos"):
        cake_amd.op_gemv_qkv_rope_bias(z(64), z(64), z((Nq, 64)), z(Nq), tab,
                                       tab, kc, kc, vt, ms, nh, nkv)
    with pytest.raises(ValueError, match="bias"):
        cake_amd.op_gemv_qkv_rope_bias(z(64), z(64), z((Nq, 64)), z(Nq + 1),
                                       tab, tab, kc, kc, vt, 0, nh, nkv)
