"""GPU engine tests (-m gpu) of qwen2 / qwen2.5: the q|k|v projection bias
through the loader, prefill (every weight format adds it in the rope + KV-store
kernel), decode (bf16: the biased fused kernel; 4-bit: split GEMV + biased
store), graph replay, chunked prefill and layer shards.

The committed fixture tests/golden/tiny_qwen2 is pinned to HF transformers'
Qwen2ForCausalLM (tools/gen_golden_qwen2.py); the two further configs are
checked against tests/qwen2_ref.Qwen2Oracle.  An engine that ignores the biases
misses the logits tests by about 1.3 relative (tests/test_bias_ref.py shows
that dropping any single one costs at least four times the limit)."""
import json
import os

import numpy as np
import pytest

import cake_amd
from oracle import Config, random_weights
from tests import qwen2_ref as qr
from tests.helpers import (fixture_weights, flatten, quantize_bf16,
                           save_safetensors_raw)
from tests.test_gpu_parity import quantized_oracle, rel_err
from tests.test_w4_engine_gpu import bf16_oracle, random_gptq_model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _write(w, cfg, biases, path, bias_dtype=np.float32, drop=()):
    """bias_dtype: a numpy dtype, or "BF16" (written through torch: numpy has
    no bfloat16)."""
    t = {k: np.ascontiguousarray(v, dtype=np.float32)
         for k, v in flatten(w, cfg).items()}
    bf16 = bias_dtype == "BF16"
    b = qr.bias_tensors(biases, cfg, np.float32 if bf16 else bias_dtype)
    t.update(b)
    for k in drop:
        del t[k]
    if not bf16:
        save_safetensors_raw(t, path)
        return
    import torch
    from safetensors.torch import save_file
    tt = {k: torch.from_numpy(v) for k, v in t.items()}
    for k in b:
        tt[k] = tt[k].to(torch.bfloat16)
    save_file(tt, path)


def _reference(cfg, w, biases):
    """The qwen2 oracle on weights rounded as the engine stores them (the
    biases stay f32 on the device)."""
    return qr.Qwen2Oracle(cfg, quantized_oracle(cfg, w).w, biases)


def _greedy_near_tie(eng, make_ref, prompt, gen, limit):
    """The project's greedy rule: every id equals the reference's until the
    first mismatch, which must be a near-tie of the reference's top two."""
    got = eng.generate_greedy(np.array(prompt, dtype=np.uint32), gen)
    toks = [int(t) for t in prompt]
    exact = 0
    for step, tok in enumerate(got):
        lg = make_ref().forward(np.array([toks], dtype=np.int64), 0)[0]
        if int(np.argmax(lg)) != int(tok):
            srt = np.sort(lg)
            gap = (srt[-1] - srt[-2]) / max(1e-9, np.max(np.abs(lg)))
            assert gap < limit, (f"token {step} diverged with top-2 gap "
                                 f"{gap:.4f}: not a bf16 near-tie")
            break
        exact += 1
        toks.append(int(tok))
    return exact


# ---- the committed fixture ------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    cfg_json, cfg, w, z = fixture_weights(GOLDEN, "tiny_qwen2")
    biases = qr.fused_biases({k[2:]: z[k] for k in z.files}, cfg)
    st = str(tmp_path_factory.mktemp("tiny_qwen2") / "model.safetensors")
    _write(w, cfg, biases, st)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=128,
                          max_batch_tokens=64)
    eng.load_safetensors(st)
    yield cfg_json, cfg, w, z, biases, st, eng
    eng.close()


def test_prefill_logits_vs_hf(tiny):
    cfg_json, cfg, w, z, biases, st, eng = tiny
    eng.reset()
    _, logits = eng.prefill(z["prompt"].astype(np.uint32), want_logits=True)
    r = rel_err(logits, z["hf_logits"])
    print(f"tiny_qwen2: prefill logits rel err vs HF {r:.3e}")
    assert r < 2e-2, f"prefill logits rel err {r} vs HF transformers"


def test_greedy_vs_reference(tiny):
    cfg_json, cfg, w, z, biases, st, eng = tiny
    gen = 12
    exact = _greedy_near_tie(eng, lambda: _reference(cfg, w, biases),
                             list(z["prompt"]), gen, 3e-2)
    assert exact >= int(0.75 * gen), f"only {exact}/{gen} exact"


def test_decode_matches_uncached_prefill(tiny):
    cfg_json, cfg, w, z, biases, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)
    eng.reset()
    first = eng.prefill(prompt)
    toks = eng.decode(3)
    seq = np.concatenate([prompt, [first], toks[:-1]]).astype(np.uint32)
    eng.reset()
    _, logits = eng.prefill(seq, want_logits=True)
    assert int(np.argmax(logits)) == int(toks[-1])


def test_graph_and_eager_agree(tiny):
    cfg_json, cfg, w, z, biases, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)
    eng.reset()                                  # fixture engine: USE_GRAPH
    g = [eng.prefill(prompt)] + list(eng.decode(8))
    e2 = cake_amd.Engine(json.dumps(cfg_json), max_seq=128,
                         max_batch_tokens=64,
                         flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
    try:
        e2.load_safetensors(st)
        e = [e2.prefill(prompt)] + list(e2.decode(8))
    finally:
        e2.close()
    assert g == e, "graph replay and eager decode disagree"


def test_chunked_prefill_and_append(tiny):
    cfg_json, cfg, w, z, biases, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)       # 17 tokens
    eng.reset()
    _, whole = eng.prefill(prompt, want_logits=True)
    small = cake_amd.Engine(json.dumps(cfg_json), max_seq=128,
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
    cfg_json, cfg, w, z, biases, st, eng = tiny
    lo = cake_amd.Engine(json.dumps(cfg_json), 0, 1, flags=0, max_seq=128,
                         max_batch_tokens=64)
    hi = cake_amd.Engine(json.dumps(cfg_json), 1, 2, flags=0, max_seq=128,
                         max_batch_tokens=64)
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
        # and the blocks are the reference's blocks
        o = _reference(cfg, w, biases)
        x = (rng.standard_normal((6, cfg.hidden_size)) * 0.05
             ).astype(np.float32)
        eng.reset()
        got = eng.forward_hidden(x, 0)
        want = o.hidden_forward(quantize_bf16(x)[None], 0, 0, 2)[0]
        assert rel_err(got, want) < 2e-2
    finally:
        lo.close()
        hi.close()


def test_init_random_is_deterministic_and_biased(tiny):
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


def test_loader_requires_the_biases(tiny, tmp_path):
    cfg_json, cfg, w, z, biases, _, _ = tiny
    name = "model.layers.1.self_attn.k_proj.bias"
    short = [b[:-1] for b in biases]             # v_proj.bias one short
    for kw, bs, msg in ((dict(drop=(name,)), biases, r"k_proj\.bias"),
                        (dict(), short, r"v_proj\.bias")):
        st = str(tmp_path / "m.safetensors")
        _write(w, cfg, bs, st, **kw)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=64,
                              max_batch_tokens=32)
        try:
            with pytest.raises(cake_amd.CakeHipError, match=msg):
                eng.load_safetensors(st)
        finally:
            eng.close()
        os.remove(st)


# ---- hd 128, G = 7: the per-head decode-attention fallback ------------------------
G7 = dict(
    model_type="qwen2", hidden_size=256, intermediate_size=512,
    vocab_size=512, num_hidden_layers=2, num_attention_heads=7,
    num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-6,
    rope_theta=1000000.0, max_position_embeddings=512,
    tie_word_embeddings=True)


@pytest.mark.parametrize("bias_dtype", ["F16", "BF16"])
def test_hd128_g7_vs_reference(tmp_path, bias_dtype):
    cfg = Config.from_json(G7)
    assert cake_amd.attn_dispatch(1, 7, 1, 128)["decode_grid_y"] == 0
    assert cake_amd.decode_dispatch(G7)["qkv"][0] == "qkv_rope"
    w = random_weights(cfg, seed=53)
    biases = qr.random_biases(cfg, seed=54)
    st = str(tmp_path / "m.safetensors")
    if bias_dtype == "F16":
        _write(w, cfg, biases, st, bias_dtype=np.float16)
        biases = [b.astype(np.float16).astype(np.float32) for b in biases]
    else:
        _write(w, cfg, biases, st, bias_dtype="BF16")
        biases = [quantize_bf16(b) for b in biases]
    eng = cake_amd.Engine(json.dumps(G7), max_seq=256, max_batch_tokens=128)
    try:
        eng.load_safetensors(st)
        prompt = np.random.default_rng(5).integers(
            0, cfg.vocab_size, size=40).astype(np.uint32)
        ref = _reference(cfg, w, biases).forward(
            prompt[None, :].astype(np.int64), 0)[0]
        _, logits = eng.prefill(prompt, want_logits=True)
        r = rel_err(logits, ref)
        print(f"qwen2 hd128 G7: prefill logits rel err {r:.3e}")
        assert r < 2e-2, f"prefill logits rel err {r}"
        exact = _greedy_near_tie(eng, lambda: _reference(cfg, w, biases),
                                 list(prompt), 6, 3e-2)
        print(f"qwen2 hd128 G7: {exact}/6 greedy ids exact")
    finally:
        eng.close()


# ---- a synthetic GPTQ checkpoint with F16 biases ----------------------------------
GPTQ = dict(
    model_type="qwen2", hidden_size=256, intermediate_size=256,
    vocab_size=512, num_hidden_layers=2, num_attention_heads=4,
    num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-6,
    rope_theta=1000000.0, max_position_embeddings=512,
    tie_word_embeddings=True,
    quantization_config=dict(quant_method="gptq", bits=4, group_size=32,
                             desc_act=False, sym=False))


def test_gptq_checkpoint_vs_reference(tmp_path):
    cfg = Config.from_json(GPTQ)
    assert cake_amd.decode_dispatch(GPTQ)["qkv"][0] == "gemv_w4"
    tensors, w = random_gptq_model(GPTQ, seed=37, f16=True)
    biases = [b.astype(np.float16).astype(np.float32)
              for b in qr.random_biases(cfg, seed=38)]
    tensors.update(qr.bias_tensors(biases, cfg, np.float16))
    st = str(tmp_path / "m.safetensors")
    save_safetensors_raw(tensors, st)
    make_ref = lambda: qr.Qwen2Oracle(cfg, bf16_oracle(cfg, w).w, biases)
    eng = cake_amd.Engine(json.dumps(GPTQ), max_seq=256, max_batch_tokens=128)
    try:
        eng.load_safetensors(st)
        prompt = np.random.default_rng(5).integers(
            0, cfg.vocab_size, size=40).astype(np.uint32)
        ref = make_ref().forward(prompt[None, :].astype(np.int64), 0)[0]
        _, logits = eng.prefill(prompt, want_logits=True)
        r = rel_err(logits, ref)
        print(f"qwen2 gptq: prefill logits rel err {r:.3e}")
        assert r < 3e-2, f"gptq prefill logits rel err {r}"
        exact = _greedy_near_tie(eng, make_ref, list(prompt), 6, 3e-2)
        print(f"qwen2 gptq: {exact}/6 greedy ids exact")
        # without its biases the same checkpoint is refused
        bad = {k: v for k, v in tensors.items()
               if k != "model.layers.0.self_attn.q_proj.bias"}
        st2 = str(tmp_path / "bad.safetensors")
        save_safetensors_raw(bad, st2)
        e2 = cake_amd.Engine(json.dumps(GPTQ), max_seq=64,
                             max_batch_tokens=32)
        try:
            with pytest.raises(cake_amd.CakeHipError,
                               match=r"layers\.0\.self_attn\.q_proj\.bias"):
                e2.load_safetensors(st2)
        finally:
            e2.close()
    finally:
        eng.close()
