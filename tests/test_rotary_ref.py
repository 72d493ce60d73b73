"""CPU tests of phi3 support: the committed fixture and its reference, the rope
tables of cake_hip_rope_tables against their float64 definition, the teeth of
the GPU op tests (tests/test_rotary_ops_gpu.py), and the host-only surface
(config refusals, kernel dispatch of the new configs, model tables).

Teeth: for every call the GPU module makes, every defect of
rotary_cases.DEFECTS that can show at the shape must move some element of the
reference by more than TWICE what the GPU test grants there (any bit where the
GPU test compares bits), in at least one of the call's input families."""
import ctypes
import json
import os

import numpy as np
import pytest

import cake_amd
from cake_amd.configs import (MODELS, PHI_MODELS, QUANT_MODELS, QWEN2_MODELS,
                              find_model, weight_bytes, weight_bytes_bf16)
from tests import phi3_ref as pr
from tests import rotary_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GPU_GATE = 2e-2                  # relative logits limit of the engine tests
SHORT_SEQ, LONG_SEQ = 32, 128    # engine max_seq of the two fixture prompts
_id = lambda c: "-".join(map(str, c))


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- fixture ----------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return pr.fixture(GOLDEN)


def _logits(fx, max_seq, toks, **kw):
    cfg_json, cfg, w, z, t = fx
    o = pr.Phi3Oracle(cfg, w, cfg_json, max_seq, **kw)
    return o.forward(np.asarray(toks)[None, :], 0)[0]


def test_fixture_is_the_issues_shape(fx):
    cfg_json, cfg, w, z, t = fx
    assert cfg_json["model_type"] == "phi3"
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size,
            cfg.num_hidden_layers, cfg.num_attention_heads,
            cfg.num_key_value_heads, cfg.hd) == (64, 128, 256, 2, 4, 2, 16)
    assert not cfg.tie_word_embeddings
    # the on-disk form
    assert cfg_json["partial_rotary_factor"] == 0.75
    assert cfg_json["original_max_position_embeddings"] == SHORT_SEQ
    assert cfg_json["max_position_embeddings"] == LONG_SEQ
    assert cfg_json["rope_scaling"]["type"] == "longrope"
    p = pr.rope_params(cfg_json)
    assert p["rd"] == 12 and len(p["longrope"]["short"]) == 6 == \
        len(p["longrope"]["long"])
    # fused tensors, bf16-representable
    assert t["model.layers.0.self_attn.qkv_proj.weight"].shape == (128, 64)
    assert t["model.layers.1.mlp.gate_up_proj.weight"].shape == (256, 64)
    assert not any("q_proj" in k or "gate_proj" in k for k in t)
    for k, v in t.items():
        assert np.array_equal(v.view(np.uint32) & 0xFFFF, np.zeros_like(
            v, dtype=np.uint32)), k
    assert len(z["prompt"]) == 17 and len(z["prompt_long"]) == 40
    assert len(z["prompt"]) + len(z["hf_gen"]) == 29 <= SHORT_SEQ


def test_reference_matches_hf_on_the_fixture(fx):
    cfg_json, cfg, w, z, t = fx
    assert _rel(_logits(fx, SHORT_SEQ, z["prompt"]), z["hf_logits"]) < 2e-4
    assert _rel(_logits(fx, LONG_SEQ, z["prompt_long"]),
                z["hf_logits_long"]) < 2e-4
    o = pr.Phi3Oracle(cfg, w, cfg_json, SHORT_SEQ)
    gen = o.generate_greedy(list(z["prompt"]), len(z["hf_gen"]))
    assert gen == [int(x) for x in z["hf_gen"]]


@pytest.mark.parametrize("defect", pr.ROPE_DEFECTS)
def test_a_wrong_rope_moves_the_logits(fx, defect):
    """Condition of the fixture: an engine with this defect misses the GPU
    gate by a factor of four at the least."""
    z = fx[3]
    if defect == "short_list":
        seq, toks, want = LONG_SEQ, z["prompt_long"], z["hf_logits_long"]
    else:
        seq, toks, want = SHORT_SEQ, z["prompt"], z["hf_logits"]
    move = _rel(_logits(fx, seq, toks, defect=defect), want)
    assert move >= 4 * GPU_GATE, (defect, move)


def test_bf16_activations_leave_headroom(fx):
    z = fx[3]
    for seq, toks, want in ((SHORT_SEQ, z["prompt"], z["hf_logits"]),
                            (LONG_SEQ, z["prompt_long"], z["hf_logits_long"])):
        assert _rel(_logits(fx, seq, toks, act_bf16=True), want) <= \
            GPU_GATE / 2


# ---- cake_hip_rope_tables vs the float64 definition ---------------------------
def _respelled(cfg_json):
    """The same config with the rotary fields inside rope_parameters."""
    c = {k: v for k, v in cfg_json.items()
         if k not in ("rope_scaling", "partial_rotary_factor",
                      "original_max_position_embeddings")}
    rs = dict(cfg_json["rope_scaling"])
    c["rope_parameters"] = dict(
        rope_type=rs.pop("type"),
        partial_rotary_factor=cfg_json["partial_rotary_factor"],
        original_max_position_embeddings=cfg_json[
            "original_max_position_embeddings"], **rs)
    return c


def _table_cases():
    with open(os.path.join(GOLDEN, "tiny_phi3.config.json")) as f:
        tiny = json.load(f)
    su = dict(tiny, rope_scaling=dict(tiny["rope_scaling"], type="su"))
    mini = PHI_MODELS["phi-4-mini"]
    return [("tiny-short", tiny, SHORT_SEQ), ("tiny-long", tiny, LONG_SEQ),
            ("tiny-rope_parameters-short", _respelled(tiny), SHORT_SEQ),
            ("tiny-rope_parameters-long", _respelled(tiny), LONG_SEQ),
            ("tiny-su-long", su, LONG_SEQ),
            ("phi-4-mini-short", mini, 4096), ("phi-4-mini-long", mini, 8192)]


@pytest.mark.parametrize("name,cfg,max_seq", _table_cases(),
                         ids=[c[0] for c in _table_cases()])
def test_rope_tables_vs_float64(name, cfg, max_seq):
    """Bound m (2^-22 |a| + 2^-22), a the angle: the frequency (power,
    reciprocal and factor product, evaluated in double and rounded once) and
    the position product give under 2^-22 relative on a (an error of da on the
    angle moves cos and sin by at most da); cosf / sinf and the product with m
    give under one ulp of a value <= m."""
    cos, sin = cake_amd.rope_tables(cfg, max_seq)
    c64, s64, a, m = pr.rope_tables64(cfg, max_seq)
    assert cos.shape == sin.shape == c64.shape == (
        max_seq, pr.rope_params(cfg)["rd"] // 2)
    assert m > 1.0
    bound = m * (2.0 ** -22 * np.abs(a) + 2.0 ** -22)
    worst = max(np.max(np.abs(cos - c64) / bound),
                np.max(np.abs(sin - s64) / bound))
    print(f"{name}: engine tables at {worst:.3f} of the bound")
    assert worst <= 1.0
    c32, s32 = pr.rope_tables32(cfg, max_seq)
    w32 = max(np.max(np.abs(c32 - c64) / bound),
              np.max(np.abs(s32 - s64) / bound))
    print(f"{name}: numpy-f32 tables at {w32:.3f} of the bound")
    assert w32 <= 1.0
    # the list in use is the one max_seq selects
    lr_ = pr.rope_params(cfg)["longrope"]
    lst = lr_["long"] if max_seq > lr_["orig"] else lr_["short"]
    inv = a[1]                           # position 1: the frequencies
    want = 1.0 / (np.array(lst) * np.power(
        float(pr.rope_params(cfg)["theta"]),
        2.0 * np.arange(len(lst)) / (2 * len(lst))))
    assert np.allclose(inv, want, rtol=1e-12)


def test_other_rope_tables_are_unchanged():
    """Full rotation, plain and llama3-scaled: the engine's tables are the
    oracle's (f32, the same formulas) to 2^-22 (|a| + 1)."""
    from oracle import Config, rope_tables
    for name in ("llama3-8b", "qwen3-0.6b", "mistral-7b"):
        cfg = MODELS[name]
        cos, sin = cake_amd.rope_tables(cfg, 256)
        oc = Config.from_json(cfg)
        oc.max_seq_len = 256
        c, s = rope_tables(oc)
        assert cos.shape == c.shape == (256, oc.hd // 2)
        a = np.arccos(np.clip(c[1].astype(np.float64), -1, 1))
        tol = 2.0 ** -22 * (np.arange(256)[:, None] * a[None, :] + 1)
        assert (np.abs(cos - c) <= tol).all() and (np.abs(sin - s) <= tol).all()


# ---- teeth: store kernels -----------------------------------------------------
@pytest.mark.parametrize("case", rc.store_cases(), ids=_id)
def test_store_teeth(case):
    nh, nkv, hd, rd, S, pos0, decode = case
    d = rc.store_inputs(*case)
    base = rc.store_ref(d, nh, nkv, hd, rd, pos0)
    assert base["qrot"][..., :rd].all() and not base["qrot"][..., rd:].any()
    fits, moved = set(), set()
    for mut in rc.DEFECTS:
        m = rc.store_ref(d, nh, nkv, hd, rd, pos0, mut)
        if m is None:
            continue
        fits.add(mut)
        if rc.store_moved(base, m, pos0, S):
            moved.add(mut)
    # q's pass-through dims are left in place by the store kernels, so a
    # defect of q's pass-through dims alone has nothing to move there
    fits -= {"q_pass_neighbour"} - moved
    assert fits - moved == set()
    gone = (nkv < 2) + (pos0 == 0 and S == 1) + 1
    assert len(fits) >= len(rc.DEFECTS) - gone


# ---- teeth: fused kernel ------------------------------------------------------
@pytest.mark.parametrize("case", rc.fused_cases(), ids=_id)
def test_fused_teeth(case):
    nh, nkv, hd, rd, K, pos = case
    fits, moved = set(), set()
    for fam in rc.FUSED_FAMILIES:
        d = rc.fused_inputs(fam, *case)
        if d["exact"]:
            assert rc.fused_sums_exact(d)
        base = rc.fused_ref(d, nh, nkv, hd, rd, pos)
        assert base["q_rot"][:, :rd].all() and not base["q_rot"][:, rd:].any()
        for mut in rc.DEFECTS:
            m = rc.fused_ref(d, nh, nkv, hd, rd, pos, mut)
            if m is None:
                continue
            fits.add(mut)
            if rc.fused_moved(base, m, d["exact"]):
                moved.add(mut)
    assert fits - moved == set()
    assert len(fits) >= len(rc.DEFECTS) - (nkv < 2) - (pos == 0)


def test_cases_are_the_issues():
    sc = rc.store_cases()
    assert {c[:4] for c in sc} == {(2, 1, 16, 12), (4, 2, 64, 48),
                                   (3, 1, 128, 96), (4, 1, 128, 32),
                                   (2, 1, 128, 4), (2, 1, 128, 124)}
    assert {(c[4], c[5]) for c in sc if not c[6]} == {
        (S, p) for S in (1, 5, 33) for p in (0, 7)}
    assert {c[5] for c in sc if c[6]} == {0, 45, 63}
    fc = rc.fused_cases()
    kbs = {cake_amd.linear_dispatch("qkv_rope", 128, c[4])["kb"] for c in fc}
    assert kbs == {1, 2, 4, 8}
    assert (24, 8, 128, 96, 3072, 45) in fc
    for nh, nkv, hd, rd, K, pos in fc:
        assert 0 < rd < hd and rd % 4 == 0 and (hd - rd) % 4 == 0
    from tests import linear_cases as lc
    for g in lc.rope_cases():
        assert {c[3] for c in fc if (c[:3] + c[4:]) == g} == {
            g[2] * 3 // 4, g[2] // 4, 4, g[2] - 4}


# ---- host-only surface --------------------------------------------------------
PINNED = {
    "phi-4": dict(qkv=("qkv_rope", 4, 4), o=("gemv_reg", 2, 4),
                  gateup=("gateup", 4, 4), down=("gemv_stream", 4, 0),
                  head=("gemv_reg", 8, 4)),
    "phi-4-mini": dict(qkv=("qkv_rope", 4, 2), o=("gemv_reg", 2, 2),
                       gateup=("gateup", 4, 2), down=("gemv_reg", 4, 4),
                       head=("gemv_reg", 8, 2)),
    "phi-4-gptq": dict(qkv=("gemv_w4", 4, 2), o=("gemv_w4", 4, 2),
                       gateup=("gateup_w4", 4, 2), down=("gemv_w4", 4, 8),
                       head=("gemv_reg", 8, 4)),
}


def test_decode_dispatch_of_the_new_configs():
    assert set(PINNED) == set(PHI_MODELS)
    for name, cfg in PHI_MODELS.items():
        assert cake_amd.decode_dispatch(cfg) == PINNED[name], name
        H, I = cfg["hidden_size"], cfg["intermediate_size"]
        hd = cfg.get("head_dim") or H // cfg["num_attention_heads"]
        Sq = cfg["num_attention_heads"] * hd
        Nq = Sq + 2 * cfg["num_key_value_heads"] * hd
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
    # partial rotary on another model type keeps the fused decode kernel
    llama = dict(MODELS["llama3-8b"], partial_rotary_factor=0.5)
    assert cake_amd.decode_dispatch(llama)["qkv"] == \
        cake_amd.decode_dispatch(MODELS["llama3-8b"])["qkv"]


def _create_code(cfg):
    h = ctypes.c_void_p()
    return cake_amd._lib.cake_hip_engine_create(
        json.dumps(cfg).encode(), 0, 1, 0, 64, 32, 0, ctypes.byref(h))


def _refused(cfg, pattern):
    assert _create_code(cfg) == 5
    msg = cake_amd._lib.cake_hip_last_error().decode()
    import re
    assert re.search(pattern, msg), msg
    with pytest.raises(cake_amd.CakeHipError, match=pattern):
        cake_amd.decode_dispatch(cfg)
    with pytest.raises(cake_amd.CakeHipError, match=pattern):
        cake_amd.rope_tables(cfg, 64)


MINI = PHI_MODELS["phi-4-mini"]


@pytest.mark.parametrize("factor", [0.0, 0.01, 0.74, 0.99, 1.5, -0.5])
def test_bad_partial_rotary_factor_is_refused(factor):
    """hd 128: rd 0, 1, 94, 126, 192, -64."""
    cfg = dict(MODELS["llama3-8b"], partial_rotary_factor=factor)
    _refused(cfg, "partial_rotary_factor")
    cfg = dict(MODELS["llama3-8b"],
               rope_parameters=dict(partial_rotary_factor=factor))
    _refused(cfg, "partial_rotary_factor")


def test_partial_rotary_with_qk_norm_or_bias_is_refused():
    for base, what in ((MODELS["qwen3-0.6b"], "QK-norm"),
                       (QWEN2_MODELS["qwen2.5-7b"], "bias")):
        cfg = dict(base, partial_rotary_factor=0.5)
        _refused(cfg, "partial_rotary_factor.*" + what)
        cake_amd.decode_dispatch(dict(base, partial_rotary_factor=1.0))


@pytest.mark.parametrize("which", ["short_factor", "long_factor"])
def test_longrope_list_lengths_are_checked(which):
    rs = dict(MINI["rope_scaling"])
    rs[which] = rs[which][:-1]
    _refused(dict(MINI, rope_scaling=rs), which + r".* 47 .* 48")
    rs.pop(which)
    _refused(dict(MINI, rope_scaling=rs), which + r".* 0 .* 48")
    # the lists follow rd, not hd
    _refused(dict(MINI, partial_rotary_factor=1.0), r"short_factor.* 48 .* 64")


def test_longrope_original_max_and_spellings():
    no_orig = {k: v for k, v in MINI.items()
               if k != "original_max_position_embeddings"}
    _refused(no_orig, "original_max_position_embeddings")
    # the dict's value wins over the top level's: 8192 > 4096 but <= 16384
    rs = dict(MINI["rope_scaling"], original_max_position_embeddings=16384)
    a = cake_amd.rope_tables(dict(MINI, rope_scaling=rs), 8192)[0]
    b = cake_amd.rope_tables(dict(no_orig, rope_scaling=rs), 8192)[0]
    assert np.array_equal(a, b)
    c64 = pr.rope_tables64(dict(MINI, rope_scaling=rs), 8192)[0]
    assert np.abs(a - c64).max() < 1e-2
    assert np.abs(a - cake_amd.rope_tables(MINI, 8192)[0]).max() > 0.5
    # factor and attention_factor are honoured
    for extra in (dict(factor=4.0), dict(attention_factor=1.25),
                  dict(factor=0.5)):
        cfg = dict(MINI, rope_scaling=dict(MINI["rope_scaling"], **extra))
        got = cake_amd.rope_tables(cfg, 4096)[0]
        c64, _, _, m = pr.rope_tables64(cfg, 4096)
        assert np.abs(got - c64).max() < 1e-3 * m
        assert abs(got[0, 0] - m) < 1e-6
    assert pr.rope_tables64(dict(MINI, rope_scaling=dict(
        MINI["rope_scaling"], factor=0.5)), 4096)[3] == 1.0
    # an unknown scaling type is ignored, as before
    y = dict(MODELS["llama3-8b"], rope_scaling=dict(type="yarn", factor=4.0))
    assert np.array_equal(
        cake_amd.rope_tables(y, 64)[0],
        cake_amd.rope_tables(dict(y, rope_scaling=None), 64)[0])


def test_phi3_config_rules():
    base = dict(PHI_MODELS["phi-4"])
    # defaults of phi4/config.rs: rope_theta 1e6, kv heads = heads
    no_theta = {k: v for k, v in base.items() if k != "rope_theta"}
    assert np.array_equal(
        cake_amd.rope_tables(no_theta, 64)[0],
        cake_amd.rope_tables(dict(base, rope_theta=1e6), 64)[0])
    mha = {k: v for k, v in base.items() if k != "num_key_value_heads"}
    assert cake_amd.decode_dispatch(mha) == cake_amd.decode_dispatch(
        dict(base, num_key_value_heads=40))
    fp8 = dict(base, quantization_config=dict(quant_method="fp8"))
    _refused(fp8, "fp8.*phi3")
    with pytest.raises(cake_amd.CakeHipError, match="multiple of 32"):
        cake_amd.rope_tables(base, 48)
    # the gptq shape rules name the fused tensors
    g = dict(PHI_MODELS["phi-4-gptq"], intermediate_size=17924)
    with pytest.raises(cake_amd.CakeHipError, match="down_proj"):
        cake_amd.decode_dispatch(g)
    g = dict(PHI_MODELS["phi-4-gptq"], hidden_size=5136)
    with pytest.raises(cake_amd.CakeHipError, match="qkv_proj"):
        cake_amd.decode_dispatch(g)


def test_tables_and_byte_counts():
    tables = (MODELS, QUANT_MODELS, QWEN2_MODELS)
    assert not any(set(PHI_MODELS) & set(t) for t in tables)
    for name, cfg in PHI_MODELS.items():
        assert find_model(name) is cfg
    assert find_model("llama3-8b") is MODELS["llama3-8b"]
    assert find_model("qwen2.5-7b") is QWEN2_MODELS["qwen2.5-7b"]
    with pytest.raises(KeyError):
        find_model("phi-3-medium")
    c = PHI_MODELS["phi-4"]
    assert (c["model_type"], c["hidden_size"], c["intermediate_size"],
            c["vocab_size"], c["num_hidden_layers"], c["num_attention_heads"],
            c["num_key_value_heads"], c["rope_theta"],
            c["max_position_embeddings"], c["tie_word_embeddings"]) == (
        "phi3", 5120, 17920, 100352, 40, 40, 10, 250000.0, 16384, False)
    m = PHI_MODELS["phi-4-mini"]
    assert (m["model_type"], m["hidden_size"], m["intermediate_size"],
            m["vocab_size"], m["num_hidden_layers"], m["num_attention_heads"],
            m["num_key_value_heads"], m["head_dim"],
            m["partial_rotary_factor"], m["rope_theta"],
            m["max_position_embeddings"],
            m["original_max_position_embeddings"],
            m["tie_word_embeddings"]) == (
        "phi3", 3072, 8192, 200064, 32, 24, 8, 128, 0.75, 10000.0, 131072,
        4096, True)
    rs = m["rope_scaling"]
    assert rs["type"] == "longrope"
    for k in ("short_factor", "long_factor"):
        assert len(rs[k]) == 48 and all(
            b > a for a, b in zip(rs[k], rs[k][1:]))
    q = PHI_MODELS["phi-4-gptq"]["quantization_config"]
    assert (q["quant_method"], q["bits"], q["group_size"],
            q["desc_act"]) == ("gptq", 4, 128, False)
    # parameter counts: 14.7 B and 3.8 B
    assert 14.6e9 < weight_bytes(c) / 2 < 14.8e9
    assert 3.8e9 < weight_bytes(m) / 2 < 3.9e9
    assert weight_bytes(c) == weight_bytes_bf16(c)
    assert weight_bytes(PHI_MODELS["phi-4-gptq"]) < weight_bytes(c) / 2.9


def test_op_entries_validate_before_any_device_call():
    z = np.zeros
    nh, nkv, hd, ms = 2, 1, 64, 64
    Nq = (nh + 2 * nkv) * hd
    kc, vt = z((nkv, ms, hd), np.float32), z((nkv, hd, ms), np.float32)
    E = cake_amd.CakeHipError
    for rd in (0, 6, 62, 68):
        tab = z((ms, rd // 2), np.float32)
        with pytest.raises(E, match="rd"):
            cake_amd.op_kv_store_pr(z((1, Nq)), tab, tab, kc, kc, vt, 0, nh,
                                    nkv, rd)
        with pytest.raises(E, match="rd"):
            cake_amd.op_gemv_qkv_rope_pr(z(64), z(64), z((Nq, 64)), tab, tab,
                                         kc, kc, vt, 0, nh, nkv, rd)
    tab = z((ms, 24), np.float32)
    with pytest.raises(E, match="QK-norm"):
        cake_amd.op_kv_store_pr(z((1, Nq)), tab, tab, kc, kc, vt, 0, nh, nkv,
                                48, q_norm=z(hd), k_norm=z(hd))
    with pytest.raises(ValueError, match="cos"):     # tables are (ms, rd/2)
        cake_amd.op_kv_store_pr(z((1, Nq)), z((ms, 32), np.float32), tab, kc,
                                kc, vt, 0, nh, nkv, 48)
    with pytest.raises(E, match="outside the cache"):
        cake_amd.op_kv_store_pr(z((1, Nq)), tab, tab, kc, kc, vt, ms, nh, nkv,
                                48)
    with pytest.raises(E, match="pos"):
        cake_amd.op_gemv_qkv_rope_pr(z(64), z(64), z((Nq, 64)), tab, tab, kc,
                                     kc, vt, ms, nh, nkv, 48)
