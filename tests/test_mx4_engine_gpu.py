"""GPU engine tests (-m gpu) of the MXFP4 path, modelled on
test_w4_engine_gpu.py: a synthetic AMD Quark checkpoint loads, prefills through
the dequant-to-scratch GEMMs, decodes through the fp4 GEMVs (eager and graph)
and shards by layer range, against the oracle on the dequantized weights
(every one exactly representable in bf16)."""
import json

import numpy as np
import pytest

import cake_amd
from oracle import Config, LayerWeights, ModelWeights
from tests import mx4_ref as mr
from tests.helpers import save_safetensors_raw
from tests import test_w4_engine_gpu as w4t   # same fixture tuple: its
from tests.test_w4_engine_gpu import bf16_oracle, rel_err  # bodies are reused

pytestmark = pytest.mark.gpu

WEIGHT = dict(dtype="fp4", qscheme="per_group", group_size=32, ch_axis=-1,
              scale_format="e8m0")
QUARK = dict(quant_method="quark", exclude=["lm_head"],
             global_quant_config=dict(
                 weight=WEIGHT, input_tensors=dict(dtype="fp4", is_dynamic=True)),
             layer_quant_config={}, layer_type_quant_config={})
BASE = dict(hidden_size=256, vocab_size=512, num_hidden_layers=2,
            max_position_embeddings=512)
CONFIGS = {
    "llama": dict(BASE, model_type="llama", intermediate_size=512,
                  num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                  rms_norm_eps=1e-5, rope_theta=500000.0,
                  tie_word_embeddings=False, quantization_config=QUARK),
    # QK-norm, tied embeddings, the one-element-list form of `weight`
    "qwen3": dict(BASE, model_type="qwen3", intermediate_size=256,
                  num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                  rms_norm_eps=1e-6, rope_theta=1000000.0,
                  tie_word_embeddings=True, quantization_config=dict(
                      QUARK, global_quant_config=dict(weight=[WEIGHT])))}
LLAMA = CONFIGS["llama"]


def random_mx4_model(cfg_json, seed):
    """(safetensors dict: U8 weight / weight_scale per projection, F32 norms
    and embedding; ModelWeights of the dequantized weights for the oracle)."""
    cfg = Config.from_json(cfg_json)
    rng = np.random.default_rng(seed)
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    hd, nh, nkv = cfg.hd, cfg.num_attention_heads, cfg.num_key_value_heads
    dense = lambda *s, base=0.0: (
        base + rng.standard_normal(s) * 0.02).astype(np.float32)
    tensors, layers = {}, []
    for i in range(cfg.num_hidden_layers):
        p, lw = f"model.layers.{i}.", {}
        for name, n, k in (("self_attn.q_proj", nh * hd, H),
                           ("self_attn.k_proj", nkv * hd, H),
                           ("self_attn.v_proj", nkv * hd, H),
                           ("self_attn.o_proj", H, nh * hd),
                           ("mlp.gate_proj", I, H), ("mlp.up_proj", I, H),
                           ("mlp.down_proj", H, I)):
            # codes have rms ~2.9, bytes 119..121 are 2^-8..2^-6: rms ~0.03
            w, s = mr.pack(rng.integers(0, 16, size=(n, k)),
                           rng.integers(119, 122, size=(n, k // 32)))
            tensors[p + name + ".weight"] = w
            tensors[p + name + ".weight_scale"] = s
            lw[name.split(".")[1]] = mr.dequant(w, s).astype(np.float32)
        norms = ["input_layernorm", "post_attention_layernorm"]
        if cfg_json["model_type"] == "qwen3":
            norms += ["q_norm", "k_norm"]
        for nm in norms:
            lw[nm] = dense(hd if "_norm" in nm else H, base=1.0)
            tensors[p + ("self_attn." if "_norm" in nm else "") + nm +
                    ".weight"] = lw[nm]
        layers.append(LayerWeights(**lw))
    embed, norm = dense(V, H), dense(H, base=1.0)
    head = embed if cfg.tie_word_embeddings else dense(V, H)
    tensors.update({"model.embed_tokens.weight": embed,
                    "model.norm.weight": norm})
    if head is not embed:
        tensors["lm_head.weight"] = head
    return tensors, ModelWeights(embed_tokens=embed, norm=norm, lm_head=head,
                                 layers=layers)


@pytest.fixture(scope="module", params=list(CONFIGS))
def mx4_model(request, tmp_path_factory):
    cfg_json = CONFIGS[request.param]
    tensors, w = random_mx4_model(cfg_json, seed=31)
    st = str(tmp_path_factory.mktemp(request.param) / "m.safetensors")
    save_safetensors_raw(tensors, st)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=256,
                          max_batch_tokens=128)
    eng.load_safetensors(st)
    yield request.param, cfg_json, Config.from_json(cfg_json), w, st, eng
    eng.close()


def test_prefill_logits_and_greedy_decode_vs_oracle(mx4_model):
    name, cfg_json, cfg, w, st, eng = mx4_model
    prompt = np.random.default_rng(5).integers(
        0, cfg.vocab_size, size=40).astype(np.uint32)
    logits_of = lambda seq: bf16_oracle(cfg, w).forward(
        np.array([seq], dtype=np.int64), 0)[0]
    eng.reset()
    first, logits = eng.prefill(prompt, want_logits=True)
    r = rel_err(logits, logits_of(list(prompt)))
    print(f"{name}: mxfp4 prefill logits rel err {r:.3e}")
    assert r < 3e-2, f"{name}: mxfp4 prefill logits rel err {r}"
    # greedy decode (fp4 GEMVs) vs the oracle's uncached forward; a mismatch
    # must be a bf16 near-tie of the oracle's top two, then stop
    seq = [int(t) for t in prompt]
    for step, tok in enumerate([int(first)] + [int(t) for t in eng.decode(5)]):
        lg = logits_of(seq)
        if int(np.argmax(lg)) != tok:
            srt = np.sort(lg)
            gap = (srt[-1] - srt[-2]) / max(1e-9, np.max(np.abs(lg)))
            assert gap < 3e-2, (f"{name}: token {step} diverged with top-2 "
                                f"gap {gap:.4f}: not a bf16 near-tie")
            break
        seq.append(tok)


def test_graph_decode_equals_eager_decode(mx4_model):
    w4t.test_graph_decode_equals_eager_decode(mx4_model)


def test_two_shard_chain_equals_monolithic(mx4_model):
    w4t.test_two_shard_chain_equals_monolithic(mx4_model)


def test_init_random_mx4_decodes_and_is_deterministic():
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


UP, O = "model.layers.1.mlp.up_proj", "model.layers.0.self_attn.o_proj"


@pytest.mark.parametrize("key,edit,msg", [
    (UP + ".weight_scale", None, r"up_proj\.weight_scale"),
    (O + ".weight", lambda a: a.astype(np.float32), r"o_proj\.weight: F32"),
    (UP + ".weight_scale", lambda a: a[:, :-1], r"up_proj\.weight_scale"),
    (UP + ".weight_scale", lambda a: np.where(np.indices(a.shape)[1] == 3,
                                              255, a).astype(np.uint8),
     r"up_proj\.weight_scale: byte 255"),
], ids=["missing_scale", "weight_f32", "scale_shape", "scale_255"])
def test_loader_errors_name_the_tensor(tmp_path, key, edit, msg):
    tensors, _ = random_mx4_model(LLAMA, seed=3)
    if edit is None:
        del tensors[key]
    else:
        tensors[key] = edit(tensors[key])
    st = str(tmp_path / "m.safetensors")
    save_safetensors_raw(tensors, st)
    eng = cake_amd.Engine(json.dumps(LLAMA), max_seq=64, max_batch_tokens=32)
    try:
        with pytest.raises(cake_amd.CakeHipError, match=msg):
            eng.load_safetensors(st)
    finally:
        eng.close()
