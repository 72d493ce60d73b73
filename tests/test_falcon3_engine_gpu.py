"""GPU engine tests (-m gpu) at head_dim 256 (Falcon3): the decode kernel
k_attn_decode_256 and the MFMA-256 prefill kernel through prefill, cached and
graph decode, chunked prefill and layer shards, for every model type and weight
format the engine runs at hd <= 128.

The committed fixture tests/golden/tiny_falcon3 is pinned to HF transformers'
LlamaForCausalLM (tools/gen_golden_falcon3.py; nh 2, nkv 1: under
CAKE_ATTN256_GB one block serves both q heads; the default is per head).  It is built so that a score over half the head, an output whose
upper half repeats the lower, or the scale of a 128-wide head each cost at
least four times the 2e-2 limit (tests/test_hd256_ref.py).  The further
configs are seeded and checked against the oracle; their q and k rows are
scaled by four for the same reason."""
import json
import os

import numpy as np
import pytest

import cake_amd
from oracle import Config, random_weights
from tests import phi3_ref as pr
from tests.falcon3_ref import Hd256Oracle
from tests.helpers import (fixture_weights, quantize_bf16, random_fp8_model,
                           save_safetensors_raw, weights_to_safetensors)
from tests.test_gpu_parity import quantized_oracle, rel_err
from tests.test_phi3_engine_gpu import _greedy_near_tie
from tests.test_w4_engine_gpu import bf16_oracle, random_gptq_model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_SEQ = 64


# ---- the committed fixture ---------------------------------------------------
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    cfg_json, cfg, w, z = fixture_weights(GOLDEN, "tiny_falcon3")
    st = str(tmp_path_factory.mktemp("tiny_falcon3") / "model.safetensors")
    weights_to_safetensors(w, cfg, st)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=MAX_SEQ,
                          max_batch_tokens=MAX_SEQ)
    eng.load_safetensors(st)
    yield cfg_json, cfg, w, z, st, eng
    eng.close()


def _ref(tiny):
    cfg_json, cfg, w = tiny[:3]
    return Hd256Oracle(cfg, w, cfg_json, MAX_SEQ)


def test_routes(tiny):
    cfg = tiny[1]
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hd
    assert hd == 256
    assert cake_amd.attn_decode_path(nh, nkv, hd, 4) == 3
    assert cake_amd.attn_decode_group(nh, nkv, hd) == 1      # the default
    assert cake_amd.attn_dispatch(17, nh, nkv, hd)["pfv"] == 1


def test_prefill_logits_vs_hf(tiny):
    cfg_json, cfg, w, z, st, eng = tiny
    eng.reset()
    _, logits = eng.prefill(z["prompt"].astype(np.uint32), want_logits=True)
    r = rel_err(logits, z["hf_logits"])
    print(f"tiny_falcon3: prefill logits rel err vs HF {r:.3e}")
    assert r < 2e-2, f"prefill logits rel err {r} vs HF transformers"


def test_greedy_on_the_grouped_route(tiny, monkeypatch):
    """CAKE_ATTN256_GB=4 (read per launch): one block serves both q heads;
    the same ids under the near-tie rule."""
    cfg_json, cfg, w, z, st, _ = tiny
    monkeypatch.setenv("CAKE_ATTN256_GB", "4")
    assert cake_amd.attn_decode_group(2, 1, 256) == 2
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=MAX_SEQ,
                          max_batch_tokens=MAX_SEQ,
                          flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
    try:
        eng.load_safetensors(st)
        exact = _greedy_near_tie(eng, lambda: _ref(tiny), list(z["prompt"]),
                                 12, 3e-2)
    finally:
        eng.close()
    assert exact >= 9, f"only {exact}/12 exact"


def test_greedy_vs_reference(tiny):
    cfg_json, cfg, w, z, st, eng = tiny
    gen = 12
    exact = _greedy_near_tie(eng, lambda: _ref(tiny), list(z["prompt"]), gen,
                             3e-2)
    assert exact >= int(0.75 * gen), f"only {exact}/{gen} exact"


def test_decode_matches_uncached_prefill(tiny):
    cfg_json, cfg, w, z, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)
    eng.reset()
    first = eng.prefill(prompt)
    toks = eng.decode(3)
    seq = np.concatenate([prompt, [first], toks[:-1]]).astype(np.uint32)
    eng.reset()
    _, logits = eng.prefill(seq, want_logits=True)
    assert int(np.argmax(logits)) == int(toks[-1])


def test_graph_and_eager_agree(tiny):
    cfg_json, cfg, w, z, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)
    eng.reset()                                  # fixture engine: USE_GRAPH
    g = [eng.prefill(prompt)] + list(eng.decode(8))
    e2 = cake_amd.Engine(json.dumps(cfg_json), max_seq=MAX_SEQ,
                         max_batch_tokens=MAX_SEQ,
                         flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
    try:
        e2.load_safetensors(st)
        e = [e2.prefill(prompt)] + list(e2.decode(8))
    finally:
        e2.close()
    assert g == e, "graph replay and eager decode disagree"


def test_chunked_prefill_and_append(tiny):
    cfg_json, cfg, w, z, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)       # 17 tokens
    eng.reset()
    _, whole = eng.prefill(prompt, want_logits=True)
    small = cake_amd.Engine(json.dumps(cfg_json), max_seq=MAX_SEQ,
                            max_batch_tokens=8)   # chunks of 8 + 8 + 1
    try:
        small.load_safetensors(st)
        _, chunked = small.prefill(prompt, want_logits=True)
        assert rel_err(chunked, whole) < 1e-3, "chunked != single-chunk"
        assert rel_err(chunked, z["hf_logits"]) < 2e-2
        small.reset()                            # 10 tokens, then 7 appended
        small.prefill(prompt[:10])
        _, appended = small.prefill(prompt[10:], want_logits=True)
        assert rel_err(appended, whole) < 1e-3, "append != single-chunk"
    finally:
        small.close()


def test_two_shard_chain_equals_monolithic(tiny):
    cfg_json, cfg, w, z, st, eng = tiny
    kw = dict(flags=0, max_seq=MAX_SEQ, max_batch_tokens=MAX_SEQ)
    lo = cake_amd.Engine(json.dumps(cfg_json), 0, 1, **kw)
    hi = cake_amd.Engine(json.dumps(cfg_json), 1, 2, **kw)
    try:
        lo.load_safetensors(st)
        hi.load_safetensors(st)
        rng = np.random.default_rng(9)
        eng.reset()
        for S, pos in ((8, 0), (1, 8)):          # a prefill, a decode step
            x = (rng.standard_normal((S, cfg.hidden_size)) * 0.05
                 ).astype(np.float32)
            ref = eng.forward_hidden_range(x, pos, 0, 2)
            a = lo.forward_hidden_range(x, pos, 0, 1)
            b = hi.forward_hidden_range(a, pos, 1, 2)
            assert np.array_equal(b, ref), (S, rel_err(b, ref))
        x = (rng.standard_normal((6, cfg.hidden_size)) * 0.05
             ).astype(np.float32)
        eng.reset()
        got = eng.forward_hidden(x, 0)
        want = _ref(tiny).hidden_forward(quantize_bf16(x)[None], 0, 0, 2)[0]
        assert rel_err(got, want) < 2e-2
    finally:
        lo.close()
        hi.close()


def test_init_random_is_deterministic(tiny):
    cfg_json = tiny[0]
    outs = []
    for seed in (1234, 1234, 99):
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=64,
                              max_batch_tokens=32)
        try:
            eng.init_random(seed=seed, scale=0.05)
            _, lg = eng.prefill(np.arange(1, 17, dtype=np.uint32),
                                want_logits=True)
            outs.append((lg, list(eng.decode(6))))
        finally:
            eng.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    assert not np.array_equal(outs[0][0], outs[2][0])
    assert np.isfinite(outs[0][0]).all()
    assert all(0 <= t < cfg_json["vocab_size"] for t in outs[0][1])


# ---- seeded configs vs the oracle, all at hd 256 ---------------------------------
def _small(model_type, nh, nkv, **kw):
    return dict(
        model_type=model_type, hidden_size=256, intermediate_size=256,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=nh,
        num_key_value_heads=nkv, head_dim=256, rms_norm_eps=1e-5,
        rope_theta=10000.0, max_position_embeddings=512,
        tie_word_embeddings=False, **kw)


SMALL = {
    "g3": _small("llama", 6, 2),
    "g4": _small("llama", 4, 1),
    "g5": _small("llama", 5, 1),                 # no group: per head
    "qwen3-qknorm": _small("qwen3", 4, 2),       # the store route
    "mistral-window16": _small("mistral", 4, 2, sliding_window=16),
    "fp8": _small("llama", 4, 2, quantization_config=dict(
        quant_method="fp8", weight_block_size=[128, 128])),
    "gptq-g32": _small("llama", 4, 2, quantization_config=dict(
        quant_method="gptq", bits=4, group_size=32, desc_act=False,
        sym=False)),
    "partial-rotary-0.5": _small("llama", 6, 2, partial_rotary_factor=0.5),
}
# CAKE_ATTN256_GB per config (None: the default, per head) and the q-heads
# per block that gives
CAP = {"g3": "4", "g4": "4", "g5": "4", "qwen3-qknorm": None,
       "mistral-window16": "4", "fp8": None, "gptq-g32": "4",
       "partial-rotary-0.5": None}
GROUP = {"g3": 3, "g4": 4, "g5": 1, "qwen3-qknorm": 1, "mistral-window16": 2,
         "fp8": 1, "gptq-g32": 2, "partial-rotary-0.5": 1}


def _model(name, cfg_json, cfg, st):
    """Writes the checkpoint; returns (make_ref, logits gate)."""
    q = cfg_json.get("quantization_config", {}).get("quant_method")
    if q == "fp8":
        tensors, w = random_fp8_model(cfg, seed=31)
        save_safetensors_raw(tensors, st)
        return (lambda: quantized_oracle(cfg, w)), 3e-2
    if q == "gptq":
        tensors, w = random_gptq_model(cfg_json, seed=31)
        save_safetensors_raw(tensors, st)
        return (lambda: bf16_oracle(cfg, w)), 3e-2
    w = random_weights(cfg, seed=61)
    for lw in w.layers:      # peakier softmax: attention errors reach the logits
        lw.q_proj = lw.q_proj * np.float32(4)
        lw.k_proj = lw.k_proj * np.float32(4)
    weights_to_safetensors(w, cfg, st)
    wq = quantized_oracle(cfg, w).w
    if "partial_rotary_factor" in cfg_json:
        return (lambda: pr.Phi3Oracle(cfg, wq, cfg_json, 256)), 2e-2
    return (lambda: quantized_oracle(cfg, w)), 2e-2


@pytest.mark.parametrize("name", list(SMALL))
def test_small_config_vs_oracle(tmp_path, name, monkeypatch):
    monkeypatch.delenv("CAKE_ATTN256_GB", raising=False)
    if CAP[name]:
        monkeypatch.setenv("CAKE_ATTN256_GB", CAP[name])
    cfg_json = SMALL[name]
    cfg = Config.from_json(cfg_json)
    nh, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
    assert cake_amd.attn_decode_group(nh, nkv, 256) == GROUP[name]
    st = str(tmp_path / "m.safetensors")
    make_ref, gate = _model(name, cfg_json, cfg, st)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=256,
                          max_batch_tokens=128)
    try:
        eng.load_safetensors(st)
        prompt = np.random.default_rng(5).integers(
            0, cfg.vocab_size, size=40).astype(np.uint32)
        ref = make_ref().forward(prompt[None, :].astype(np.int64), 0)[0]
        _, logits = eng.prefill(prompt, want_logits=True)
        r = rel_err(logits, ref)
        print(f"{name}: prefill logits rel err {r:.3e}")
        assert r < gate, f"prefill logits rel err {r}"
        exact = _greedy_near_tie(eng, make_ref, list(prompt), 6, 3e-2)
        print(f"{name}: {exact}/6 greedy ids exact")
        # cached decode against an uncached prefill
        eng.reset()
        first = eng.prefill(prompt)
        toks = eng.decode(3)
        seq = np.concatenate([prompt, [first], toks[:-1]]).astype(np.uint32)
        eng.reset()
        _, lg = eng.prefill(seq, want_logits=True)
        want = make_ref().forward(seq[None, :].astype(np.int64), 0)[0]
        assert rel_err(lg, want) < gate
        srt = np.sort(want)
        if (srt[-1] - srt[-2]) / np.max(np.abs(want)) >= 3e-2:
            assert int(np.argmax(want)) == int(toks[-1])
    finally:
        eng.close()
