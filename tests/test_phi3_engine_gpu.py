"""GPU engine tests (-m gpu) of phi3 (Phi-3 / Phi-4-mini / Phi-4): the fused
checkpoint tensors through the loader (bf16 and GPTQ), partial rotary through
prefill (the store kernel with the real rd), decode (bf16: k_gemv_qkv_rope_pr;
4-bit: split GEMV + store), graph replay, chunked prefill and layer shards, and
the LongRoPE tables with the list chosen by the engine's max_seq.

The committed fixture tests/golden/tiny_phi3 is pinned to HF transformers'
Phi3ForCausalLM (tools/gen_golden_phi3.py): the 17-token prompt against HF on
its short list (engine max_seq 32 = original_max_position_embeddings), the
40-token prompt against HF on its long list (engine max_seq 128).  It is built
so that rotating all head dims, a missing attention factor, ignored short
factors or the wrong list each cost at least four times the 2e-2 limit
(tests/test_rotary_ref.py).  The further configs are checked against
tests/phi3_ref.Phi3Oracle."""
import json
import os

import numpy as np
import pytest

import cake_amd
from oracle import Config, random_weights
from tests import phi3_ref as pr
from tests.helpers import (flatten, quantize_bf16, save_safetensors_raw,
                           weights_to_safetensors)
from tests.test_gpu_parity import quantized_oracle, rel_err
from tests.test_w4_engine_gpu import bf16_oracle, random_gptq_model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHORT_SEQ, LONG_SEQ = 32, 128


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


def _write_fused(w, cfg, path, drop=(), edit=None):
    t = pr.fused_tensors({k: np.ascontiguousarray(v, dtype=np.float32)
                          for k, v in flatten(w, cfg).items()}, cfg)
    for k in drop:
        del t[k]
    if edit:
        edit(t)
    save_safetensors_raw(t, path)


# ---- the committed fixture ------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    cfg_json, cfg, w, z, t = pr.fixture(GOLDEN)
    st = str(tmp_path_factory.mktemp("tiny_phi3") / "model.safetensors")
    save_safetensors_raw(t, st)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=SHORT_SEQ,
                          max_batch_tokens=SHORT_SEQ)
    eng.load_safetensors(st)
    yield cfg_json, cfg, w, z, st, eng
    eng.close()


def _ref(tiny, max_seq=SHORT_SEQ):
    cfg_json, cfg, w = tiny[:3]
    return pr.Phi3Oracle(cfg, w, cfg_json, max_seq)


def test_prefill_logits_vs_hf_short_list(tiny):
    cfg_json, cfg, w, z, st, eng = tiny
    eng.reset()
    _, logits = eng.prefill(z["prompt"].astype(np.uint32), want_logits=True)
    r = rel_err(logits, z["hf_logits"])
    print(f"tiny_phi3: prefill logits rel err vs HF (short list) {r:.3e}")
    assert r < 2e-2, f"prefill logits rel err {r} vs HF transformers"


def test_prefill_logits_vs_hf_long_list(tiny):
    cfg_json, cfg, w, z, st, _ = tiny
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=LONG_SEQ,
                          max_batch_tokens=64)
    try:
        eng.load_safetensors(st)
        _, logits = eng.prefill(z["prompt_long"].astype(np.uint32),
                                want_logits=True)
    finally:
        eng.close()
    r = rel_err(logits, z["hf_logits_long"])
    print(f"tiny_phi3: prefill logits rel err vs HF (long list) {r:.3e}")
    assert r < 2e-2, f"prefill logits rel err {r} vs HF transformers"


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
    e2 = cake_amd.Engine(json.dumps(cfg_json), max_seq=SHORT_SEQ,
                         max_batch_tokens=SHORT_SEQ,
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
    small = cake_amd.Engine(json.dumps(cfg_json), max_seq=SHORT_SEQ,
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
    kw = dict(flags=0, max_seq=SHORT_SEQ, max_batch_tokens=SHORT_SEQ)
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
        # and the blocks are the reference's blocks
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


def test_loader_requires_the_fused_tensors(tiny, tmp_path):
    cfg_json, cfg, w = tiny[:3]
    qkv = "model.layers.1.self_attn.qkv_proj.weight"
    gu = "model.layers.0.mlp.gate_up_proj.weight"

    def short(t):
        t[gu] = np.ascontiguousarray(t[gu][:-1])

    def write_split(path):
        weights_to_safetensors(w, cfg, path)

    cases = ((lambda p: _write_fused(w, cfg, p, drop=(qkv,)),
              r"layers\.1\.self_attn\.qkv_proj\.weight"),
             (write_split, r"layers\.0\.self_attn\.qkv_proj\.weight"),
             (lambda p: _write_fused(w, cfg, p, edit=short),
              r"layers\.0\.mlp\.gate_up_proj\.weight"))
    for write, msg in cases:
        st = str(tmp_path / "m.safetensors")
        write(st)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=64,
                              max_batch_tokens=32)
        try:
            with pytest.raises(cake_amd.CakeHipError, match=msg):
                eng.load_safetensors(st)
        finally:
            eng.close()
        os.remove(st)


# ---- seeded small configs vs the reference ---------------------------------------
def _small(model_type, nh, nkv, hd, factor, H=256):
    return dict(
        model_type=model_type, hidden_size=H, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=nh,
        num_key_value_heads=nkv, head_dim=hd, rms_norm_eps=1e-5,
        rope_theta=10000.0, partial_rotary_factor=factor,
        max_position_embeddings=512, tie_word_embeddings=True)


SMALL = {
    # hd 64 / rd 48, G = 3
    "phi3-hd64-rd48-g3": _small("phi3", 6, 2, 64, 0.75),
    # Phi-4-mini's head geometry: hd 128 / rd 96, G = 3 takes the per-head
    # decode attention, and decode runs k_gemv_qkv_rope_pr
    "phi3-hd128-rd96-g3": _small("phi3", 6, 2, 128, 0.75),
    # partial rotary is no phi3 privilege: split tensors, factor 0.5
    "llama-hd64-rd32": _small("llama", 4, 2, 64, 0.5),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_small_config_vs_reference(tmp_path, name):
    cfg_json = SMALL[name]
    cfg = Config.from_json(cfg_json)
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hd
    assert cake_amd.decode_dispatch(cfg_json)["qkv"][0] == "qkv_rope"
    if name == "phi3-hd128-rd96-g3":
        assert cake_amd.attn_dispatch(1, nh, nkv, hd)["decode_grid_y"] == 0
    w = random_weights(cfg, seed=61)
    st = str(tmp_path / "m.safetensors")
    if cfg_json["model_type"] == "phi3":
        _write_fused(w, cfg, st)
    else:
        weights_to_safetensors(w, cfg, st)
    wq = quantized_oracle(cfg, w).w
    make_ref = lambda: pr.Phi3Oracle(cfg, wq, cfg_json, 256)
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
        assert r < 2e-2, f"prefill logits rel err {r}"
        # a full rotation would be somewhere else
        full = pr.Phi3Oracle(cfg, wq, cfg_json, 256, defect="full_rotation"
                             ).forward(prompt[None, :].astype(np.int64), 0)[0]
        print(f"{name}: a full rotation is {rel_err(full, ref):.3e} away")
        exact = _greedy_near_tie(eng, make_ref, list(prompt), 6, 3e-2)
        print(f"{name}: {exact}/6 greedy ids exact")
        # decode (the fused kernel) against an uncached prefill
        eng.reset()
        first = eng.prefill(prompt)
        toks = eng.decode(3)
        seq = np.concatenate([prompt, [first], toks[:-1]]).astype(np.uint32)
        eng.reset()
        _, lg = eng.prefill(seq, want_logits=True)
        want = make_ref().forward(seq[None, :].astype(np.int64), 0)[0]
        assert rel_err(lg, want) < 2e-2
        srt = np.sort(want)
        if (srt[-1] - srt[-2]) / np.max(np.abs(want)) >= 3e-2:
            assert int(np.argmax(want)) == int(toks[-1])
    finally:
        eng.close()


def test_split_route_under_bf16_splitnorm(tmp_path, monkeypatch):
    """CAKE_BF16_SPLITNORM=1 sends a partial-rotary model down norm + GEMV +
    store (the A/B leg of the fused kernel); it decodes the reference's ids
    too."""
    name = "phi3-hd128-rd96-g3"
    cfg_json = SMALL[name]
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=61)
    st = str(tmp_path / "m.safetensors")
    _write_fused(w, cfg, st)
    wq = quantized_oracle(cfg, w).w
    make_ref = lambda: pr.Phi3Oracle(cfg, wq, cfg_json, 256)
    prompt = np.random.default_rng(5).integers(0, cfg.vocab_size, size=40)
    monkeypatch.setenv("CAKE_BF16_SPLITNORM", "1")
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=256,
                          max_batch_tokens=128)
    monkeypatch.delenv("CAKE_BF16_SPLITNORM")
    try:
        eng.load_safetensors(st)
        eng.set_stats(True)
        eng.prefill(prompt.astype(np.uint32))
        eng.decode(2)
        eng.sync()
        eng.set_stats(False)
        assert "rope_store" in eng.kernel_stats()["kernels"]
        exact = _greedy_near_tie(eng, make_ref, list(prompt), 6, 3e-2)
        print(f"{name} split route: {exact}/6 greedy ids exact")
    finally:
        eng.close()


# ---- a synthetic fused GPTQ checkpoint --------------------------------------------
GPTQ = dict(
    model_type="phi3", hidden_size=256, intermediate_size=256,
    vocab_size=512, num_hidden_layers=2, num_attention_heads=4,
    num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-5,
    rope_theta=10000.0, partial_rotary_factor=0.75,
    max_position_embeddings=512, tie_word_embeddings=True,
    quantization_config=dict(quant_method="gptq", bits=4, group_size=32,
                             desc_act=False, sym=False))


def _fuse_gptq(tensors, cfg):
    """Split-name AutoGPTQ tensors in phi3's names: qweight (K/8, N), qzeros
    (G, N/8) and scales (G, N) all concatenate along the output axis."""
    out = {k: v for k, v in tensors.items()
           if not any(s in k for s in ("q_proj", "k_proj", "v_proj",
                                       "gate_proj", "up_proj"))}
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        for fused, parts in (("self_attn.qkv_proj",
                              [f"self_attn.{n}_proj" for n in "qkv"]),
                             ("mlp.gate_up_proj",
                              ["mlp.gate_proj", "mlp.up_proj"])):
            for suf in (".qweight", ".qzeros", ".scales"):
                out[p + fused + suf] = np.ascontiguousarray(np.concatenate(
                    [tensors[p + n + suf] for n in parts], axis=1))
    return out


def test_gptq_checkpoint_vs_reference(tmp_path):
    cfg = Config.from_json(GPTQ)
    assert cake_amd.decode_dispatch(GPTQ)["qkv"][0] == "gemv_w4"
    split, w = random_gptq_model(GPTQ, seed=41, f16=True)
    tensors = _fuse_gptq(split, cfg)
    st = str(tmp_path / "m.safetensors")
    save_safetensors_raw(tensors, st)
    wq = bf16_oracle(cfg, w).w             # embedding and norms as stored
    make_ref = lambda: pr.Phi3Oracle(cfg, wq, GPTQ, 256)
    eng = cake_amd.Engine(json.dumps(GPTQ), max_seq=256, max_batch_tokens=128)
    try:
        eng.load_safetensors(st)
        prompt = np.random.default_rng(5).integers(
            0, cfg.vocab_size, size=40).astype(np.uint32)
        ref = make_ref().forward(prompt[None, :].astype(np.int64), 0)[0]
        _, logits = eng.prefill(prompt, want_logits=True)
        r = rel_err(logits, ref)
        print(f"phi3 gptq: prefill logits rel err {r:.3e}")
        assert r < 3e-2, f"gptq prefill logits rel err {r}"
        exact = _greedy_near_tie(eng, make_ref, list(prompt), 6, 3e-2)
        print(f"phi3 gptq: {exact}/6 greedy ids exact")
        # the split-name checkpoint is refused, naming the fused tensor
        st2 = str(tmp_path / "split.safetensors")
        save_safetensors_raw(split, st2)
        e2 = cake_amd.Engine(json.dumps(GPTQ), max_seq=64,
                             max_batch_tokens=32)
        try:
            with pytest.raises(cake_amd.CakeHipError,
                               match=r"layers\.0\.self_attn\.qkv_proj"):
                e2.load_safetensors(st2)
        finally:
            e2.close()
    finally:
        eng.close()
