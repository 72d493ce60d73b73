"""GPU engine tests (-m gpu) of the gemma3 family on the committed fixture
tests/golden/tiny_gemma3, which is pinned to HF transformers'
Gemma3ForCausalLM (tools/gen_golden_gemma3.py): layers sliding, full, sliding
with window 8 under a 17-token prompt, head_dim 256, query_pre_attn_scalar 128,
a linear global rope and a second theta for the local one.  Each way of
getting the family wrong that tests/gemma3_ref.DEFECTS lists costs at least
four times the 2e-2 limit used here (tests/test_gemma3_ref.py).

The checkpoint goes through a temporary safetensors file; max_seq is 64."""
import json
import os

import numpy as np
import pytest

import cake_amd
from tests import gemma3_ref as gr
from tests.helpers import quantize_bf16, save_safetensors_raw
from tests.test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_SEQ = 64
PLAIN = cake_amd.HAS_EMBED | cake_amd.HAS_HEAD       # no USE_GRAPH


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    cfg, t, z = gr.fixture(GOLDEN)
    st = str(tmp_path_factory.mktemp("tiny_gemma3") / "model.safetensors")
    save_safetensors_raw(t, st)
    eng = cake_amd.Engine(json.dumps(cfg), max_seq=MAX_SEQ,
                          max_batch_tokens=MAX_SEQ)
    eng.load_safetensors(st)
    yield cfg, t, z, st, eng
    eng.close()


def _ref(tiny, **kw):
    return gr.Gemma3Oracle(tiny[0], tiny[1], MAX_SEQ, **kw)


def _embedded(tiny, ids):
    """The rows the engine's embedding kernels produce for ids."""
    o = _ref(tiny, act_bf16=True)
    return o.embed(np.asarray(ids, dtype=np.int64))


def _head_logits(tiny, hidden_row):
    """The model's own head on the host: final norm, tied lm_head.  Hidden
    states are judged through it against HF's logits at the logits gate: with
    no final norm and a model 32 wide, raw hidden states of random inputs move
    by 1e-2 to 8e-2 under bf16 activations alone (the reference's own
    act_bf16 run says so), while on the prompt's embeddings and through the
    head the generator holds that estimate to half the gate."""
    o = _ref(tiny)
    x = o.norm(hidden_row[None, None, :].astype(np.float32),
               "model.norm.weight")
    return x[0, 0] @ tiny[1]["model.embed_tokens.weight"].T


def test_prefill_logits_vs_hf(tiny):
    cfg, t, z, st, eng = tiny
    eng.reset()
    _, logits = eng.prefill(z["prompt"].astype(np.uint32), want_logits=True)
    r = rel_err(logits, z["hf_logits"])
    print(f"tiny_gemma3: prefill logits rel err vs HF {r:.3e}")
    assert r < 2e-2, f"prefill logits rel err {r} vs HF transformers"


def test_greedy_ids_exact(tiny):
    cfg, t, z, st, eng = tiny
    got = eng.generate_greedy(z["prompt"].astype(np.uint32), len(z["hf_gen"]))
    assert [int(x) for x in got] == [int(x) for x in z["hf_gen"]]


def test_decode_steps_past_the_window(tiny):
    """Cached decode at positions 17.. (window 8) against an uncached prefill
    of the same sequence, in tokens and, through forward_hidden with one row
    (the decode route), in hidden states against the oracle."""
    cfg, t, z, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)
    eng.reset()
    first = eng.prefill(prompt)
    toks = eng.decode(5)
    seq = np.concatenate([prompt, [first], toks[:-1]]).astype(np.uint32)
    eng.reset()
    _, logits = eng.prefill(seq, want_logits=True)
    want = _ref(tiny).forward(seq[None, :].astype(np.int64), 0)[0]
    assert rel_err(logits, want) < 2e-2
    assert int(np.argmax(logits)) == int(toks[-1])
    # the decode route in numbers: layers through forward_hidden, 16 rows as
    # a prefill and the 17th alone (one row runs the decode kernels, at
    # position 16 with window 8), then the head on the host, against HF
    x = _embedded(tiny, z["prompt"])
    eng.reset()
    eng.forward_hidden(x[:16], 0)
    last = eng.forward_hidden(x[16:17], 16)
    r = rel_err(_head_logits(tiny, last[0]), z["hf_logits"])
    print(f"decode route at pos 16: logits rel err vs HF {r:.3e}")
    assert r < 2e-2


def test_graph_and_eager_agree(tiny):
    cfg, t, z, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)
    eng.reset()                                  # fixture engine: USE_GRAPH
    g = [eng.prefill(prompt)] + list(eng.decode(11))
    e2 = cake_amd.Engine(json.dumps(cfg), max_seq=MAX_SEQ,
                         max_batch_tokens=MAX_SEQ, flags=PLAIN)
    try:
        e2.load_safetensors(st)
        e = [e2.prefill(prompt)] + list(e2.decode(11))
    finally:
        e2.close()
    assert g == e, "graph replay and eager decode disagree"
    assert [int(x) for x in g] == [int(x) for x in z["hf_gen"]]


@pytest.mark.parametrize("bt", [4, 16], ids=["below-window", "across-window"])
def test_chunked_prefill(tiny, bt):
    cfg, t, z, st, eng = tiny
    prompt = z["prompt"].astype(np.uint32)       # 17 tokens, window 8
    eng.reset()
    _, whole = eng.prefill(prompt, want_logits=True)
    small = cake_amd.Engine(json.dumps(cfg), max_seq=MAX_SEQ,
                            max_batch_tokens=bt)
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


def test_two_shards_equal_monolithic(tiny):
    cfg, t, z, st, eng = tiny
    kw = dict(flags=0, max_seq=MAX_SEQ, max_batch_tokens=MAX_SEQ)
    lo = cake_amd.Engine(json.dumps(cfg), 0, 2, **kw)
    hi = cake_amd.Engine(json.dumps(cfg), 2, 3, **kw)
    try:
        lo.load_safetensors(st)
        hi.load_safetensors(st)
        rng = np.random.default_rng(9)
        eng.reset()
        for S, pos in ((12, 0), (1, 12)):        # a prefill, a decode step
            x = rng.standard_normal((S, cfg["hidden_size"])).astype(np.float32)
            ref = eng.forward_hidden_range(x, pos, 0, 3)
            a = lo.forward_hidden_range(x, pos, 0, 2)
            b = hi.forward_hidden_range(a, pos, 2, 3)
            assert np.array_equal(b, ref), (S, rel_err(b, ref))
        x = _embedded(tiny, z["prompt"])
        eng.reset()
        ref = eng.forward_hidden(x, 0)
        b = hi.forward_hidden_range(lo.forward_hidden_range(x, 0, 0, 2), 0, 2,
                                    3)
        assert np.array_equal(b, ref)
        r = rel_err(_head_logits(tiny, b[-1]), z["hf_logits"])
        print(f"two shards on the prompt: logits rel err vs HF {r:.3e}")
        assert r < 2e-2
    finally:
        lo.close()
        hi.close()


def test_nested_checkpoint_and_config(tiny, tmp_path):
    """model_type gemma3 with text_config, tensors under
    language_model.model. beside a vision tensor: the same logits."""
    cfg, t, z, st, eng = tiny
    eng.reset()
    _, whole = eng.prefill(z["prompt"].astype(np.uint32), want_logits=True)
    for prefix in ("language_model.model.", "model.language_model."):
        nested = {prefix + k[len("model."):]: v for k, v in t.items()}
        nested["vision_tower.vision_model.post_layernorm.weight"] = \
            np.ones(8, dtype=np.float32)
        path = str(tmp_path / (prefix.replace(".", "_") + ".safetensors"))
        save_safetensors_raw(nested, path)
        cj = dict(model_type="gemma3", text_config={
            k: v for k, v in cfg.items() if k != "model_type"})
        e2 = cake_amd.Engine(json.dumps(cj), max_seq=MAX_SEQ,
                             max_batch_tokens=MAX_SEQ)
        try:
            e2.load_safetensors(path)
            _, lg = e2.prefill(z["prompt"].astype(np.uint32),
                               want_logits=True)
        finally:
            e2.close()
        assert np.array_equal(lg, whole), prefix


def test_init_random_runs(tiny):
    cfg = tiny[0]
    outs = []
    for seed in (1234, 1234, 99):
        eng = cake_amd.Engine(json.dumps(cfg), max_seq=64,
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
    assert all(0 <= t < cfg["vocab_size"] for t in outs[0][1])


def test_missing_post_norm_tensor_is_named(tiny, tmp_path):
    cfg, t, z, st, eng = tiny
    name = "model.layers.1.post_feedforward_layernorm.weight"
    path = str(tmp_path / "missing.safetensors")
    save_safetensors_raw({k: v for k, v in t.items() if k != name}, path)
    e2 = cake_amd.Engine(json.dumps(cfg), max_seq=MAX_SEQ,
                         max_batch_tokens=MAX_SEQ)
    try:
        with pytest.raises(cake_amd.CakeHipError, match=name.replace(".", r"\.")):
            e2.load_safetensors(path)
    finally:
        e2.close()


@pytest.mark.parametrize("q", [
    dict(quant_method="fp8", weight_block_size=[128, 128]),
    dict(quant_method="gptq", bits=4, group_size=128, desc_act=False)],
    ids=["fp8", "gptq"])
def test_quantized_gemma3_is_refused(tiny, q):
    cfg = dict(tiny[0], quantization_config=q)
    with pytest.raises(cake_amd.CakeHipError,
                       match=f"quant_method {q['quant_method']} with "
                             "model_type gemma3"):
        cake_amd.Engine(json.dumps(cfg), max_seq=MAX_SEQ,
                        max_batch_tokens=MAX_SEQ)


def test_sampling_and_stats_families(tiny):
    """Temperature sampling runs, set_sampling_ex keeps its rules, and the
    new launches are booked under their own family names."""
    cfg, t, z, st, _ = tiny
    eng = cake_amd.Engine(json.dumps(cfg), max_seq=MAX_SEQ,
                          max_batch_tokens=MAX_SEQ, flags=PLAIN)
    try:
        eng.load_safetensors(st)
        eng.set_sampling(0.8, seed=5)
        eng.prefill(z["prompt"].astype(np.uint32))
        assert all(0 <= int(x) < cfg["vocab_size"] for x in eng.decode(4))
        eng.set_sampling(0.0)
        eng.reset()
        eng.set_stats(True)
        eng.prefill(z["prompt"].astype(np.uint32))
        eng.decode(2)
        fams = eng.kernel_stats()["kernels"]
    finally:
        eng.close()
    L = cfg["num_hidden_layers"]
    assert fams["postnorm_add_pf"]["launches"] == 2 * L
    assert fams["gelu_mul"]["launches"] == L
    assert fams["postnorm_add"]["launches"] == 2 * 2 * L
    assert fams["gemv_gateup_gelu"]["launches"] == 2 * L
    assert "gemv_gateup" not in fams and "silu_mul" not in fams


def test_vocab_above_the_sampler_cap(tiny):
    """4B and up: vocab 262208 is above the top-k / top-p sampler's 2^18.
    Create, greedy and temperature work; set_sampling_ex keeps its refusal."""
    cfg = dict(tiny[0], vocab_size=262208)
    eng = cake_amd.Engine(json.dumps(cfg), max_seq=MAX_SEQ,
                          max_batch_tokens=MAX_SEQ)
    try:
        eng.init_random(seed=7, scale=0.05)
        prompt = np.array([5, 262207, 77, 131072], dtype=np.uint32)
        first, lg = eng.prefill(prompt, want_logits=True)
        assert lg.shape == (262208,) and np.isfinite(lg).all()
        assert first == int(np.argmax(lg))
        assert all(0 <= int(x) < 262208 for x in eng.decode(3))
        eng.set_sampling(0.7, seed=3)
        eng.reset()
        eng.prefill(prompt)
        assert all(0 <= int(x) < 262208 for x in eng.decode(3))
        with pytest.raises(cake_amd.CakeHipError, match="vocab <= 262144"):
            eng.set_sampling_ex(0.7, top_k=40)
    finally:
        eng.close()
