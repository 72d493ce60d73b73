"""GPU engine tests (-m gpu) of the GPTQ 4-bit path: a synthetic AutoGPTQ
checkpoint (I32 qweight / qzeros, F16 scales) loads, prefills through the
dequant-to-scratch GEMMs, decodes through the in-register-dequant GEMVs (eager
and graph), and shards by layer range -- against the oracle on the
bf16-rounded dequantized weights, modelled on test_fp8_engine_parity."""
import json
import os

import numpy as np
import pytest

import cake_amd
from oracle import Config, LayerWeights, ModelWeights, OracleModel
from tests import w4_ref as wr
from tests.helpers import quantize_bf16, save_safetensors_raw

pytestmark = pytest.mark.gpu

LLAMA = dict(
    model_type="llama", hidden_size=256, intermediate_size=512,
    vocab_size=512, num_hidden_layers=2, num_attention_heads=2,
    num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-5,
    rope_theta=500000.0, max_position_embeddings=512,
    tie_word_embeddings=False,
    quantization_config=dict(quant_method="gptq", bits=4, group_size=128,
                             desc_act=False, sym=False))
QWEN3 = dict(
    model_type="qwen3", hidden_size=256, intermediate_size=256,
    vocab_size=512, num_hidden_layers=2, num_attention_heads=4,
    num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-6,
    rope_theta=1000000.0, max_position_embeddings=512,
    tie_word_embeddings=True,
    quantization_config=dict(quant_method="gptq", bits=4, group_size=32,
                             desc_act=False, sym=False))
CONFIGS = {"llama": (LLAMA, False), "qwen3": (QWEN3, True)}


def rel_err(a, b):
    return np.max(np.abs(a - b)) / max(1e-9, np.max(np.abs(b)))


def random_gptq_model(cfg_json, seed=7, f16=False):
    """Synthetic AutoGPTQ model: returns (tensors dict for safetensors: I32
    qweight / qzeros and F16 scales per projection, norms and embedding F32
    or (f16=True) F16; ModelWeights of the bf16-rounded dequantized weights
    for the oracle)."""
    cfg = Config.from_json(cfg_json)
    rng = np.random.default_rng(seed)
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    hd, nh, nkv = cfg.hd, cfg.num_attention_heads, cfg.num_key_value_heads
    g = cfg_json["quantization_config"]["group_size"]
    dt = np.float16 if f16 else np.float32

    def dense(*shape, base=0.0):
        return (base + rng.standard_normal(shape) * 0.02).astype(dt)

    tensors, layers = {}, []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        parts = {}
        for name, n, k in (("self_attn.q_proj", nh * hd, H),
                           ("self_attn.k_proj", nkv * hd, H),
                           ("self_attn.v_proj", nkv * hd, H),
                           ("self_attn.o_proj", H, nh * hd),
                           ("mlp.gate_proj", I, H),
                           ("mlp.up_proj", I, H),
                           ("mlp.down_proj", H, I)):
            q = rng.integers(0, 16, size=(k, n))
            z = rng.integers(0, 16, size=(k // g, n))
            # (q - z - 1) has rms ~6.5: weights of rms ~0.03
            s = (0.005 * 2.0 ** rng.uniform(-0.5, 0.5, size=(k // g, n))
                 ).astype(np.float16)
            qw, qz, sc = wr.pack_gptq(q, z, s.astype(np.float64))
            tensors[p + name + ".qweight"] = qw
            tensors[p + name + ".qzeros"] = qz
            tensors[p + name + ".scales"] = s
            # ignored when present (gptq.rs does the same)
            tensors[p + name + ".g_idx"] = (np.arange(k) // g).astype(np.int32)
            parts[name] = quantize_bf16(
                wr.dequant(qw, qz, sc, g).astype(np.float32))
        ln1, ln2 = dense(H, base=1.0), dense(H, base=1.0)
        tensors[p + "input_layernorm.weight"] = ln1
        tensors[p + "post_attention_layernorm.weight"] = ln2
        qn = kn = None
        if cfg_json["model_type"] == "qwen3":
            qn, kn = dense(hd, base=1.0), dense(hd, base=1.0)
            tensors[p + "self_attn.q_norm.weight"] = qn
            tensors[p + "self_attn.k_norm.weight"] = kn
        f = lambda a: None if a is None else a.astype(np.float32)
        layers.append(LayerWeights(
            input_layernorm=f(ln1), post_attention_layernorm=f(ln2),
            q_proj=parts["self_attn.q_proj"], k_proj=parts["self_attn.k_proj"],
            v_proj=parts["self_attn.v_proj"], o_proj=parts["self_attn.o_proj"],
            gate_proj=parts["mlp.gate_proj"], up_proj=parts["mlp.up_proj"],
            down_proj=parts["mlp.down_proj"], q_norm=f(qn), k_norm=f(kn)))
    embed, norm = dense(V, H), dense(H, base=1.0)
    tensors["model.embed_tokens.weight"] = embed
    tensors["model.norm.weight"] = norm
    head = embed
    if not cfg.tie_word_embeddings:
        head = dense(V, H)
        tensors["lm_head.weight"] = head
    w = ModelWeights(embed_tokens=embed.astype(np.float32),
                     norm=norm.astype(np.float32),
                     lm_head=head.astype(np.float32), layers=layers)
    return tensors, w


def bf16_oracle(cfg, w):
    """The oracle on weights rounded as the engine stores them."""
    import copy
    w2 = copy.deepcopy(w)
    w2.embed_tokens = quantize_bf16(w2.embed_tokens)
    w2.norm = quantize_bf16(w2.norm)
    w2.lm_head = quantize_bf16(w2.lm_head)
    for lw in w2.layers:
        for f in ("input_layernorm", "post_attention_layernorm", "q_norm",
                  "k_norm"):
            if getattr(lw, f) is not None:
                setattr(lw, f, quantize_bf16(getattr(lw, f)))
    return OracleModel(cfg, w2)


@pytest.fixture(scope="module", params=list(CONFIGS))
def gptq_model(request, tmp_path_factory):
    cfg_json, f16 = CONFIGS[request.param]
    tensors, w = random_gptq_model(cfg_json, seed=31, f16=f16)
    st = str(tmp_path_factory.mktemp(request.param) / "m.safetensors")
    save_safetensors_raw(tensors, st)
    cfg = Config.from_json(cfg_json)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=256,
                          max_batch_tokens=128)
    eng.load_safetensors(st)
    yield request.param, cfg_json, cfg, w, st, eng
    eng.close()


def test_prefill_logits_and_greedy_decode_vs_oracle(gptq_model):
    name, cfg_json, cfg, w, st, eng = gptq_model
    oracle = bf16_oracle(cfg, w)
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, cfg.vocab_size, size=40).astype(np.uint32)
    ref = oracle.forward(prompt[None, :].astype(np.int64), 0)[0]
    eng.reset()
    first, logits = eng.prefill(prompt, want_logits=True)
    r = rel_err(logits, ref)
    print(f"{name}: gptq prefill logits rel err {r:.3e}")
    assert r < 3e-2, f"{name}: gptq prefill logits rel err {r}"
    # greedy decode (4-bit GEMVs) vs the oracle's uncached forward; a
    # mismatch must be a bf16 near-tie of the oracle's top two, then stop
    toks = [int(first)] + [int(t) for t in eng.decode(5)]
    seq = [int(t) for t in prompt]
    for step, tok in enumerate(toks):
        o2 = bf16_oracle(cfg, w)
        lg = o2.forward(np.array([seq], dtype=np.int64), 0)[0]
        if int(np.argmax(lg)) != tok:
            srt = np.sort(lg)
            gap = (srt[-1] - srt[-2]) / max(1e-9, np.max(np.abs(lg)))
            assert gap < 3e-2, (f"{name}: token {step} diverged with top-2 "
                                f"gap {gap:.4f}: not a bf16 near-tie")
            break
        seq.append(tok)


def test_graph_decode_equals_eager_decode(gptq_model):
    name, cfg_json, cfg, w, st, eng = gptq_model
    prompt = np.random.default_rng(6).integers(
        0, cfg.vocab_size, size=24).astype(np.uint32)
    eng.reset()                                  # fixture engine: USE_GRAPH
    g = [eng.prefill(prompt)] + list(eng.decode(8))
    e2 = cake_amd.Engine(json.dumps(cfg_json), max_seq=256,
                         max_batch_tokens=128,
                         flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
    try:
        e2.load_safetensors(st)
        e = [e2.prefill(prompt)] + list(e2.decode(8))
    finally:
        e2.close()
    assert g == e, f"{name}: graph replay and eager decode disagree"


def test_two_shard_chain_equals_monolithic(gptq_model):
    name, cfg_json, cfg, w, st, eng = gptq_model
    lo = cake_amd.Engine(json.dumps(cfg_json), 0, 1, flags=0, max_seq=256,
                         max_batch_tokens=128)
    hi = cake_amd.Engine(json.dumps(cfg_json), 1, 2, flags=0, max_seq=256,
                         max_batch_tokens=128)
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
            assert np.array_equal(b, ref), (name, S, rel_err(b, ref))
    finally:
        lo.close()
        hi.close()


def test_init_random_gptq_decodes_and_is_deterministic():
    outs = []
    for _ in range(2):
        eng = cake_amd.Engine(json.dumps(LLAMA), max_seq=128,
                              max_batch_tokens=64)
        try:
            eng.init_random(seed=1234, scale=0.05)
            prompt = np.arange(1, 17, dtype=np.uint32)
            outs.append([eng.prefill(prompt)] + list(eng.decode(8)))
        finally:
            eng.close()
    assert outs[0] == outs[1] and len(outs[0]) == 9
    assert all(0 <= t < LLAMA["vocab_size"] for t in outs[0])


def test_loader_errors_name_the_tensor(tmp_path):
    tensors, _ = random_gptq_model(LLAMA, seed=3)
    E = cake_amd.CakeHipError
    name = "model.layers.1.mlp.up_proj"
    missing = {k: v for k, v in tensors.items() if k != name + ".qzeros"}
    bad = dict(tensors)
    bad[name + ".scales"] = tensors[name + ".scales"][:, :-8]
    bad_dt = dict(tensors)
    bad_dt["model.layers.0.self_attn.o_proj.qweight"] = tensors[
        "model.layers.0.self_attn.o_proj.qweight"].astype(np.float32)
    for t, msg in ((missing, r"up_proj\.qzeros"), (bad, r"up_proj\.scales"),
                   (bad_dt, r"o_proj\.qweight")):
        st = str(tmp_path / "m.safetensors")
        save_safetensors_raw(t, st)
        eng = cake_amd.Engine(json.dumps(LLAMA), max_seq=64,
                              max_batch_tokens=32)
        try:
            with pytest.raises(E, match=msg):
                eng.load_safetensors(st)
        finally:
            eng.close()
        os.remove(st)
