"""GPU parity tests (-m gpu): the gfx950 kernels and the engine against the
oracle (oracle/__init__.py, itself pinned to HF transformers golden vectors).

Comparison protocol: the engine stores bf16 and accumulates f32; the oracle
is run on bf16-QUANTIZED weights (tests/helpers.quantize_bf16) so the
remaining difference is activation rounding only.  Tolerances are stated per
test.
"""
import json

import numpy as np
import pytest

import cake_amd
from oracle import Config, OracleModel, random_weights, rope_tables
from tests.helpers import (fixture_weights, quantize_bf16,
                           weights_to_safetensors, flatten)

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    return np.max(np.abs(a - b)) / max(1e-9, np.max(np.abs(b)))


def quantized_oracle(cfg, w):
    import copy
    w2 = copy.deepcopy(w)
    w2.embed_tokens = quantize_bf16(w2.embed_tokens)
    w2.norm = quantize_bf16(w2.norm)
    w2.lm_head = quantize_bf16(w2.lm_head)
    for lw in w2.layers:
        for f in ("input_layernorm", "post_attention_layernorm", "q_proj",
                  "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
                  "down_proj", "q_norm", "k_norm"):
            v = getattr(lw, f)
            if v is not None:
                setattr(lw, f, quantize_bf16(v))
    return OracleModel(cfg, w2)


# ---------------------------------------------------------------------------
# op-level kernels vs oracle formulas
# ---------------------------------------------------------------------------
def test_op_rms_norm():
    from oracle import rms_norm
    rng = np.random.default_rng(0)
    x = rng.standard_normal((33, 4096)).astype(np.float32)
    w = rng.standard_normal(4096).astype(np.float32)
    got = cake_amd.op_rms_norm(x, w, eps=1e-5)
    ref = rms_norm(quantize_bf16(x), quantize_bf16(w), 1e-5)
    assert rel_err(got, ref) < 1e-2


def test_op_silu_mul():
    from oracle import silu_mul
    rng = np.random.default_rng(1)
    g = (rng.standard_normal(100000) * 3).astype(np.float32)
    u = rng.standard_normal(100000).astype(np.float32)
    got = cake_amd.op_silu_mul(g, u)
    ref = silu_mul(quantize_bf16(g), quantize_bf16(u))
    assert rel_err(got, ref) < 1e-2


def test_op_rope():
    from oracle import rope
    rng = np.random.default_rng(2)
    b, h, s, d = 1, 8, 17, 128
    x = rng.standard_normal((b, h, s, d)).astype(np.float32)
    cfg = Config(hidden_size=1024, intermediate_size=1, vocab_size=1,
                 num_hidden_layers=1, num_attention_heads=8,
                 num_key_value_heads=8, head_dim=d, rope_theta=500000.0,
                 max_seq_len=s)
    cos, sin = rope_tables(cfg)
    got = cake_amd.op_rope(x, cos, sin)
    ref = rope(quantize_bf16(x), cos, sin)
    assert rel_err(got, ref) < 1e-2


def test_op_gemv_m1():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 4096)).astype(np.float32)
    w = rng.standard_normal((1000, 4096)).astype(np.float32)  # N tail (not %8)
    got = cake_amd.op_linear(x, w)
    ref = quantize_bf16(x) @ quantize_bf16(w).T
    assert rel_err(got, ref) < 1e-2


def test_op_gemv_small_k():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 64)).astype(np.float32)
    w = rng.standard_normal((24, 64)).astype(np.float32)
    got = cake_amd.op_linear(x, w)
    ref = quantize_bf16(x) @ quantize_bf16(w).T
    assert rel_err(got, ref) < 1e-2


@pytest.mark.parametrize("M,N,K", [
    (128, 128, 64),        # single tile
    (256, 384, 256),       # multiple tiles
    (200, 260, 128),       # M and N tails
    (2048, 1536, 4096),    # prefill-like shape
    (33, 128256 // 16, 64),  # wide-N-ish
    (2048, 28672, 4096),   # gate_up prefill shape (hand-written: 256^2)
    (300, 51300, 256),     # hand-written: 256^2 with M and N tails
    (256, 384, 96),        # ragged K (% 64 != 0): masked tail tile (128^2)
    (200, 300, 40),        # ragged K smaller than one 64-wide tile (128^2)
])
def test_op_gemm(M, N, K):
    """The product dispatch (op_linear: hipBLASLt first for all of these
    shapes) AND the hand-written kernel the policy keeps behind the library
    for the shape, forced through the explicit-variant entry.  Sharper
    per-variant checks live in test_linear_ops_gpu.py."""
    # asymmetric random operands (transpose-detecting — guide §5.4 rule 16)
    rng = np.random.default_rng(M * 7 + N)
    x = rng.standard_normal((M, K)).astype(np.float32) * 0.5
    w = rng.standard_normal((N, K)).astype(np.float32) * 0.5
    got = cake_amd.op_linear(x, w)
    ref = quantize_bf16(x) @ quantize_bf16(w).T
    # bf16 inputs, f32 accumulate: error grows ~sqrt(K) * 2^-8
    assert rel_err(got, ref) < 2e-2
    variant = cake_amd.linear_dispatch("gemm", N, K, M=M)["variant"]
    ours, guards, ran = cake_amd.op_gemm(x, w, variant)
    assert ran == variant
    assert (guards == cake_amd.OP_SENTINEL).all()
    assert rel_err(ours, ref) < 2e-2


# ---------------------------------------------------------------------------
# engine vs oracle on the committed golden fixtures
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["tiny_llama3", "tiny_qwen3", "tiny_mistral", "tiny_qwen3swa"])
def fixture_engine(request, tmp_path_factory):
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "golden")
    cfg_json, cfg, w, z = fixture_weights(golden, request.param)
    td = tmp_path_factory.mktemp(request.param)
    st = str(td / "model.safetensors")
    weights_to_safetensors(w, cfg, st)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=128,
                          max_batch_tokens=64)
    eng.load_safetensors(st)
    yield request.param, cfg, w, z, eng
    eng.close()


def test_engine_prefill_logits_vs_oracle(fixture_engine):
    name, cfg, w, z, eng = fixture_engine
    oracle = quantized_oracle(cfg, w)
    prompt = z["prompt"]
    ref = oracle.forward(prompt[None, :], 0)[0]
    eng.reset()
    _, logits = eng.prefill(prompt.astype(np.uint32), want_logits=True)
    r = rel_err(logits, ref)
    assert r < 2e-2, f"{name}: prefill logits rel err {r}"


def test_engine_greedy_vs_oracle(fixture_engine):
    """Greedy ids vs oracle.  With random tiny weights, exact argmax may
    legitimately flip when the oracle's top-2 gap is inside bf16 noise; we
    require every mismatch to be such a near-tie and >=75% exact."""
    name, cfg, w, z, eng = fixture_engine
    oracle = quantized_oracle(cfg, w)
    prompt = list(z["prompt"])
    gen = 12
    ref = oracle.generate_greedy(prompt, gen)
    got = eng.generate_greedy(np.array(prompt, dtype=np.uint32), gen)
    exact = 0
    toks = list(prompt)
    for step, (a, b) in enumerate(zip(got, ref)):
        if a == b:
            exact += 1
            toks.append(b)
            continue
        # near-tie check at the first divergence, then stop comparing
        o2 = quantized_oracle(cfg, w)
        o2.reset()
        logits = o2.forward(np.array([toks], dtype=np.int64), 0)[0]
        srt = np.sort(logits)
        gap = srt[-1] - srt[-2]
        scale = max(1e-9, np.max(np.abs(logits)))
        assert gap / scale < 3e-2, (
            f"{name}: token {step} diverged ({a} vs {b}) with top-2 gap "
            f"{gap / scale:.4f} — not a bf16 near-tie")
        break
    assert exact >= int(0.75 * gen), f"{name}: only {exact}/{gen} exact"


def test_engine_decode_matches_uncached_prefill(fixture_engine):
    """KV-cached decode == uncached full forward (cache.rs:184-210
    property), on the engine itself."""
    name, cfg, w, z, eng = fixture_engine
    prompt = z["prompt"].astype(np.uint32)
    eng.reset()
    first = eng.prefill(prompt)
    toks = eng.decode(3)
    seq = np.concatenate([prompt, [first], toks[:-1]]).astype(np.uint32)
    eng.reset()
    _, logits = eng.prefill(seq, want_logits=True)
    assert int(np.argmax(logits)) == int(toks[-1]), (
        f"{name}: cached decode diverges from uncached forward")


def test_engine_forward_hidden_block_parity(fixture_engine):
    """Forwarder::forward unit: blocks [0, L) on raw hidden states
    (cake/mod.rs:519-540), prefill shape then a decode step."""
    name, cfg, w, z, eng = fixture_engine
    oracle = quantized_oracle(cfg, w)
    rng = np.random.default_rng(9)
    S = 12
    x = (rng.standard_normal((S, cfg.hidden_size)) * 0.05).astype(np.float32)
    ref = oracle.hidden_forward(quantize_bf16(x)[None], 0, 0,
                                cfg.num_hidden_layers)[0]
    eng.reset()
    got = eng.forward_hidden(x, 0)
    assert rel_err(got, ref) < 2e-2, f"{name}: prefill block parity"
    # decode step at index_pos = S
    x1 = (rng.standard_normal((1, cfg.hidden_size)) * 0.05).astype(np.float32)
    ref1 = oracle.hidden_forward(quantize_bf16(x1)[None], S, 0,
                                 cfg.num_hidden_layers)[0]
    got1 = eng.forward_hidden(x1, S)
    assert rel_err(got1, ref1) < 2e-2, f"{name}: decode block parity"


def test_engine_graph_and_eager_agree(fixture_engine):
    name, cfg, w, z, eng = fixture_engine
    prompt = z["prompt"].astype(np.uint32)
    # graph path (fixture engine has USE_GRAPH)
    eng.reset()
    first = eng.prefill(prompt)
    g = [first] + list(eng.decode(6))
    # eager path
    e2 = cake_amd.Engine(json.dumps(
        json.load(open(_cfgpath(name)))), max_seq=128, max_batch_tokens=64,
        flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
    try:
        import tempfile, os
        with tempfile.TemporaryDirectory() as td:
            st = os.path.join(td, "m.safetensors")
            weights_to_safetensors(w, cfg, st)
            e2.load_safetensors(st)
        first2 = e2.prefill(prompt)
        e = [first2] + list(e2.decode(6))
    finally:
        e2.close()
    assert g == e, f"{name}: graph replay and eager decode disagree"


def _cfgpath(name):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        f"{name}.config.json")


# ---------------------------------------------------------------------------
# sharded pipeline on one GPU (two engines, layer ranges chained) — the
# §8e property without needing 2 physical GPUs
# ---------------------------------------------------------------------------
def test_sharded_hidden_chain_matches_full():
    import tempfile, os
    cfg_json = dict(
        model_type="llama", hidden_size=128, intermediate_size=256,
        vocab_size=256, num_hidden_layers=4, num_attention_heads=4,
        num_key_value_heads=2, head_dim=32, rms_norm_eps=1e-5,
        rope_theta=10000.0, max_position_embeddings=128,
        tie_word_embeddings=False)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=11)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        full = cake_amd.Engine(json.dumps(cfg_json), max_seq=64,
                               max_batch_tokens=32,
                               flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
        full.load_safetensors(st)
        lo_eng = cake_amd.Engine(json.dumps(cfg_json), 0, 2, flags=0,
                                 max_seq=64, max_batch_tokens=32)
        lo_eng.load_safetensors(st)
        hi_eng = cake_amd.Engine(json.dumps(cfg_json), 2, 4, flags=0,
                                 max_seq=64, max_batch_tokens=32)
        hi_eng.load_safetensors(st)
        try:
            rng = np.random.default_rng(5)
            S = 8
            x = (rng.standard_normal((S, cfg.hidden_size)) * 0.05
                 ).astype(np.float32)
            ref = full.forward_hidden(x, 0)
            a = lo_eng.forward_hidden(x, 0)
            b = hi_eng.forward_hidden(a, 0)
            assert rel_err(b, ref) < 5e-3
            # and a decode step after
            x1 = (rng.standard_normal((1, cfg.hidden_size)) * 0.05
                  ).astype(np.float32)
            ref1 = full.forward_hidden(x1, S)
            a1 = lo_eng.forward_hidden(x1, S)
            b1 = hi_eng.forward_hidden(a1, S)
            assert rel_err(b1, ref1) < 5e-3
        finally:
            full.close()
            lo_eng.close()
            hi_eng.close()


def test_hd128_mfma_prefill_parity():
    """head_dim=128 routes prefill attention through the MFMA flash kernel —
    check it against the oracle on ragged S (tile tails, multi-workgroup)
    and that a decode step after it stays consistent."""
    import tempfile, os
    cfg_json = dict(
        model_type="llama", hidden_size=256, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=2,
        num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-5,
        rope_theta=500000.0, max_position_embeddings=1024,
        tie_word_embeddings=False)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=23)
    oracle = quantized_oracle(cfg, w)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=1024,
                              max_batch_tokens=512)
        eng.load_safetensors(st)
        try:
            rng = np.random.default_rng(3)
            for S in (1, 2, 31, 32, 33, 77, 300):
                prompt = rng.integers(0, cfg.vocab_size,
                                      size=S).astype(np.uint32)
                oracle.reset()
                ref = oracle.forward(prompt[None, :].astype(np.int64), 0)[0]
                eng.reset()
                _, logits = eng.prefill(prompt, want_logits=True)
                r = rel_err(logits, ref)
                assert r < 2e-2, f"S={S}: prefill logits rel err {r}"
            # decode after a prefill that ends mid-tile
            prompt = rng.integers(0, cfg.vocab_size, size=45).astype(np.uint32)
            oracle.reset()
            ref_toks = oracle.generate_greedy(list(prompt), 5)
            got = eng2_greedy(eng, prompt, 5)
            assert sum(a == b for a, b in zip(got, ref_toks)) >= 4
        finally:
            eng.close()


def eng2_greedy(eng, prompt, n):
    eng.reset()
    first = eng.prefill(prompt)
    return [first] + list(eng.decode(n - 1))


def test_chunked_prefill_parity():
    """Prompts longer than max_batch_tokens prefill in chunks (the engine's
    pos0-offset path, mirroring cake's whole-prompt forward in pieces):
    results must equal a single-chunk prefill and the oracle."""
    import tempfile, os
    cfg_json = dict(
        model_type="llama", hidden_size=256, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=2,
        num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-5,
        rope_theta=500000.0, max_position_embeddings=1024,
        tie_word_embeddings=False)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=41)
    oracle = quantized_oracle(cfg, w)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        big = cake_amd.Engine(json.dumps(cfg_json), max_seq=512,
                              max_batch_tokens=512)
        big.load_safetensors(st)
        small = cake_amd.Engine(json.dumps(cfg_json), max_seq=512,
                                max_batch_tokens=48)  # forces 48+48+4 chunks
        small.load_safetensors(st)
        try:
            rng = np.random.default_rng(17)
            prompt = rng.integers(0, cfg.vocab_size, size=100).astype(
                np.uint32)
            _, l_big = big.prefill(prompt, want_logits=True)
            _, l_small = small.prefill(prompt, want_logits=True)
            assert rel_err(l_small, l_big) < 1e-3, "chunked != single-chunk"
            ref = oracle.forward(prompt[None, :].astype(np.int64), 0)[0]
            assert rel_err(l_small, ref) < 2e-2
        finally:
            big.close()
            small.close()


def test_long_context_decode_parity():
    """Multi-sub-tile decode attention (the tiled split-KV kernel's rescale
    across 128-position sub-tiles): with CAKE_NCHUNK=2 and a 300-token
    context, each chunk spans 2 sub-tiles.  Decode logits must match the
    uncached forward and the oracle."""
    import os as _os
    import tempfile
    _os.environ["CAKE_NCHUNK"] = "2"
    try:
        cfg_json = dict(
            model_type="llama", hidden_size=256, intermediate_size=512,
            vocab_size=512, num_hidden_layers=2, num_attention_heads=2,
            num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-5,
            rope_theta=500000.0, max_position_embeddings=1024,
            tie_word_embeddings=False)
        cfg = Config.from_json(cfg_json)
        w = random_weights(cfg, seed=77)
        oracle = quantized_oracle(cfg, w)
        with tempfile.TemporaryDirectory() as td:
            st = _os.path.join(td, "m.safetensors")
            weights_to_safetensors(w, cfg, st)
            eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=512,
                                  max_batch_tokens=512)
            eng.load_safetensors(st)
            try:
                rng = np.random.default_rng(13)
                prompt = rng.integers(0, cfg.vocab_size,
                                      size=300).astype(np.uint32)
                first = eng.prefill(prompt)
                toks = eng.decode(4)
                # engine self-consistency: cached decode == uncached forward
                seq = np.concatenate([prompt, [first], toks[:-1]]).astype(
                    np.uint32)
                eng.reset()
                _, lg = eng.prefill(seq, want_logits=True)
                assert int(np.argmax(lg)) == int(toks[-1])
                # oracle parity on the logits after the long context
                oracle.reset()
                ref = oracle.forward(seq[None, :].astype(np.int64), 0)[0]
                assert rel_err(lg, ref) < 2e-2
            finally:
                eng.close()
    finally:
        del _os.environ["CAKE_NCHUNK"]


def test_adaptive_nchunk_recapture():
    """Crossing the 1024-context threshold mid-decode drops and re-captures
    the decode graph with a larger split-KV chunk count (engine.hip
    want_nchunk) and re-zeros the arrival counters.  Decode across the
    boundary must stay consistent with the uncached forward and the
    oracle."""
    import os
    import tempfile
    cfg_json = dict(
        model_type="llama", hidden_size=256, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=2,
        num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-5,
        rope_theta=500000.0, max_position_embeddings=4096,
        tie_word_embeddings=False)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=177)
    oracle = quantized_oracle(cfg, w)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=2048,
                              max_batch_tokens=1024)
        eng.load_safetensors(st)
        try:
            rng = np.random.default_rng(31)
            prompt = rng.integers(0, cfg.vocab_size,
                                  size=990).astype(np.uint32)
            first = eng.prefill(prompt)
            # 140 graph-replayed steps: host_pos crosses 1024 at the s=63
            # sync point -> re-capture with a larger chunk count
            toks = eng.decode(140)
            seq = np.concatenate([prompt, [first], toks[:-1]]).astype(
                np.uint32)
            eng.reset()
            _, lg = eng.prefill(seq, want_logits=True)
            assert int(np.argmax(lg)) == int(toks[-1])
            oracle.reset()
            ref = oracle.forward(seq[None, :].astype(np.int64), 0)[0]
            assert rel_err(lg, ref) < 2e-2
        finally:
            eng.close()


def test_sharded_window_boundary_chain():
    """Sharding an interleaved-window model so the shard boundary splits
    the full layer from the windowed one: per-layer windows must key on
    the ABSOLUTE layer index (LayerDev.idx = layer_lo + i), not the
    shard-local index.  4 layers, max_window_layers=2: engine A holds
    [0,2) (full), engine B holds [2,4) (windowed); prompt 80 > window 32
    so the window actually bites."""
    import os
    import tempfile
    cfg_json = dict(
        model_type="llama", hidden_size=128, intermediate_size=256,
        vocab_size=256, num_hidden_layers=4, num_attention_heads=4,
        num_key_value_heads=2, head_dim=32, rms_norm_eps=1e-5,
        rope_theta=10000.0, max_position_embeddings=512,
        tie_word_embeddings=False, sliding_window=32,
        use_sliding_window=True, max_window_layers=2)
    cfg = Config.from_json(cfg_json)
    assert cfg.layer_windows == (None, None, 32, 32)
    w = random_weights(cfg, seed=23)
    oracle = quantized_oracle(cfg, w)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        full = cake_amd.Engine(json.dumps(cfg_json), max_seq=256,
                               max_batch_tokens=128,
                               flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
        full.load_safetensors(st)
        lo_eng = cake_amd.Engine(json.dumps(cfg_json), 0, 2, flags=0,
                                 max_seq=256, max_batch_tokens=128)
        lo_eng.load_safetensors(st)
        hi_eng = cake_amd.Engine(json.dumps(cfg_json), 2, 4, flags=0,
                                 max_seq=256, max_batch_tokens=128)
        hi_eng.load_safetensors(st)
        try:
            rng = np.random.default_rng(9)
            prompt = rng.integers(0, cfg.vocab_size,
                                  size=80).astype(np.uint32)
            # monolithic engine vs oracle
            _, lg = full.prefill(prompt, want_logits=True)
            ref = oracle.forward(prompt[None, :].astype(np.int64), 0)[0]
            assert rel_err(lg, ref) < 2e-2
            # sharded chain on raw hidden states == monolithic blocks
            S = 80
            x = (rng.standard_normal((S, cfg.hidden_size)) * 0.05
                 ).astype(np.float32)
            full2 = full  # blocks [0,4) via forward_hidden need a fresh
            # position: use separate engines' own caches at index 0
            a = lo_eng.forward_hidden(x, 0)
            b = hi_eng.forward_hidden(a, 0)
            # reference: a 4-layer full-range engine without head flags
            mono = cake_amd.Engine(json.dumps(cfg_json), 0, 4, flags=0,
                                   max_seq=256, max_batch_tokens=128)
            mono.load_safetensors(st)
            try:
                refh = mono.forward_hidden(x, 0)
                assert rel_err(b, refh) < 5e-3
            finally:
                mono.close()
        finally:
            full.close()
            lo_eng.close()
            hi_eng.close()


def test_gqa_ratio8_hd128_parity():
    """GQA ratio 8 (the 70B/32B head layout: nh/nkv = 8) with hd=128 —
    exercises the kvh = h/8 mapping in the decode and MFMA-prefill
    kernels, which the ratio-2 golden fixtures never touch."""
    import os
    import tempfile
    cfg_json = dict(
        model_type="llama", hidden_size=256, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=8,
        num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-5,
        rope_theta=500000.0, max_position_embeddings=1024,
        tie_word_embeddings=False)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=271)
    oracle = quantized_oracle(cfg, w)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=512,
                              max_batch_tokens=256)
        eng.load_safetensors(st)
        try:
            rng = np.random.default_rng(17)
            prompt = rng.integers(0, cfg.vocab_size,
                                  size=75).astype(np.uint32)
            first, lg = eng.prefill(prompt, want_logits=True)
            ref = oracle.forward(prompt[None, :].astype(np.int64), 0)[0]
            assert rel_err(lg, ref) < 2e-2
            toks = eng.decode(6)
            seq = np.concatenate([prompt, [first], toks[:-1]]).astype(
                np.uint32)
            eng.reset()
            _, lg2 = eng.prefill(seq, want_logits=True)
            assert int(np.argmax(lg2)) == int(toks[-1])
            oracle.reset()
            ref2 = oracle.forward(seq[None, :].astype(np.int64), 0)[0]
            assert rel_err(lg2, ref2) < 2e-2
        finally:
            eng.close()


@pytest.mark.parametrize("ratio,window", [(4, 0), (1, 0), (4, 96), (2, 0)])
def test_gqa_grouped_decode_hd128_parity(ratio, window):
    """hd=128 GQA geometries route decode attention through the GQA-grouped
    LDS-staged kernel (k_attn_decode_g): ratio 4 = GB4/subg1 (the 8B
    layout), ratio 1 = the GB1 residue path, ratio 2 = GB2, plus a
    sliding-window case; prompt > 2 tiles exercises ragged 64-position
    tile edges and the multi-chunk combine."""
    import os
    import tempfile
    cfg_json = dict(
        model_type="llama" if window == 0 else "mistral",
        hidden_size=256, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2,
        num_attention_heads=2 * ratio, num_key_value_heads=2,
        head_dim=128, rms_norm_eps=1e-5,
        rope_theta=500000.0, max_position_embeddings=1024,
        tie_word_embeddings=False)
    if window:
        cfg_json["sliding_window"] = window
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=411 + ratio + window)
    oracle = quantized_oracle(cfg, w)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=512,
                              max_batch_tokens=256)
        eng.load_safetensors(st)
        try:
            rng = np.random.default_rng(23 + ratio)
            prompt = rng.integers(0, cfg.vocab_size,
                                  size=150).astype(np.uint32)
            first, lg = eng.prefill(prompt, want_logits=True)
            ref = oracle.forward(prompt[None, :].astype(np.int64), 0)[0]
            assert rel_err(lg, ref) < 2e-2
            toks = eng.decode(8)
            # decode-vs-uncached-prefill self-consistency (exact argmax)
            seq = np.concatenate([prompt, [first], toks[:-1]]).astype(
                np.uint32)
            eng.reset()
            _, lg2 = eng.prefill(seq, want_logits=True)
            assert int(np.argmax(lg2)) == int(toks[-1])
            oracle.reset()
            ref2 = oracle.forward(seq[None, :].astype(np.int64), 0)[0]
            assert rel_err(lg2, ref2) < 2e-2
        finally:
            eng.close()


@pytest.mark.parametrize("plen", [1500, 3800])
def test_grouped_decode_large_nchunk_parity(plen):
    """Long contexts under the NATURAL chunk policy: plen 1500 -> nchunk 24
    (the <=32 direct ILP combine), plen 3800 -> nchunk 64 (the staged
    acquire+LDS combine) — both compared against the oracle and the
    engine's own uncached forward.  The short-prompt tests never leave
    nchunk <= 8."""
    import os
    import tempfile
    cfg_json = dict(
        model_type="llama", hidden_size=256, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=8,
        num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5,
        rope_theta=500000.0, max_position_embeddings=4096,
        tie_word_embeddings=False)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=88 + plen)
    oracle = quantized_oracle(cfg, w)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=4096,
                              max_batch_tokens=2048)
        eng.load_safetensors(st)
        try:
            rng = np.random.default_rng(plen)
            prompt = rng.integers(0, cfg.vocab_size,
                                  size=plen).astype(np.uint32)
            first = eng.prefill(prompt)
            toks = eng.decode(4)
            seq = np.concatenate([prompt, [first], toks[:-1]]).astype(
                np.uint32)
            eng.reset()
            _, lg = eng.prefill(seq, want_logits=True)
            assert int(np.argmax(lg)) == int(toks[-1])
            oracle.reset()
            ref = oracle.forward(seq[None, :].astype(np.int64), 0)[0]
            assert rel_err(lg, ref) < 2e-2
        finally:
            eng.close()


def test_max_seq_guard():
    cfg_json = dict(
        model_type="llama", hidden_size=64, intermediate_size=128,
        vocab_size=128, num_hidden_layers=1, num_attention_heads=4,
        num_key_value_heads=2, head_dim=16, max_position_embeddings=64)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=32,
                          max_batch_tokens=16)
    eng.init_random(seed=1)
    try:
        with pytest.raises(cake_amd.CakeHipError, match="max_seq"):
            eng.prefill(np.zeros(40, dtype=np.uint32))
        eng.reset()
        eng.prefill(np.zeros(8, dtype=np.uint32))
        with pytest.raises(cake_amd.CakeHipError, match="max_seq"):
            eng.decode(30)
    finally:
        eng.close()


def test_fp8_engine_parity():
    """fp8 (e4m3fn + blockwise scale_inv) weights: engine in-kernel dequant
    GEMVs (decode) and dequant-to-scratch GEMMs (prefill) vs the oracle on
    the dequantized weights (utils/fp8.rs:42-64 semantics)."""
    import tempfile, os
    from tests.helpers import random_fp8_model, save_safetensors_raw
    cfg_json = dict(
        model_type="llama", hidden_size=256, intermediate_size=256,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=2,
        num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-5,
        rope_theta=500000.0, max_position_embeddings=512,
        tie_word_embeddings=False,
        quantization_config=dict(quant_method="fp8",
                                 weight_block_size=[128, 128]))
    cfg = Config.from_json(cfg_json)
    tensors, w = random_fp8_model(cfg, seed=31)
    oracle = quantized_oracle(cfg, w)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        save_safetensors_raw(tensors, st)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=256,
                              max_batch_tokens=128)
        eng.load_safetensors(st)
        try:
            rng = np.random.default_rng(5)
            prompt = rng.integers(0, cfg.vocab_size, size=40).astype(np.uint32)
            ref = oracle.forward(prompt[None, :].astype(np.int64), 0)[0]
            first, logits = eng.prefill(prompt, want_logits=True)
            r = rel_err(logits, ref)
            assert r < 3e-2, f"fp8 prefill logits rel err {r}"
            # decode steps consistent with uncached forward
            toks = eng.decode(3)
            seq = np.concatenate([prompt, [first], toks[:-1]]).astype(
                np.uint32)
            eng.reset()
            _, lg = eng.prefill(seq, want_logits=True)
            assert int(np.argmax(lg)) == int(toks[-1])
        finally:
            eng.close()


def test_full_size_8b_determinism_and_graph_parity():
    """Full-size property test (tier framing §3: size-independent properties
    at BASELINE's full sizes): Llama-3-8B random-init — (a) two engines with
    the same seed generate identical ids; (b) hipGraph replay == eager; (c)
    a reset reproduces the same generation bit-exactly."""
    from cake_amd.configs import LLAMA3_8B
    rng = np.random.default_rng(99)
    prompt = rng.integers(0, LLAMA3_8B["vocab_size"], size=64).astype(
        np.uint32)
    a = cake_amd.Engine(json.dumps(LLAMA3_8B), max_seq=512,
                        max_batch_tokens=256)
    a.init_random()
    b = cake_amd.Engine(json.dumps(LLAMA3_8B), max_seq=512,
                        max_batch_tokens=256,
                        flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)  # eager
    b.init_random()
    try:
        ga = a.generate_greedy(prompt, 17)
        gb = b.generate_greedy(prompt, 17)
        assert ga == gb, "graph replay and eager decode disagree at 8B"
        ga2 = a.generate_greedy(prompt, 17)
        assert ga == ga2, "reset + regenerate is not bit-deterministic"
    finally:
        a.close()
        b.close()


def test_wire_worker_over_tcp_matches_local():
    """The literal drop-in story (§8f item 4): the model's second half runs
    in a wire worker behind cake's TCP protocol; the master-side chain
    (local shard -> WireClient Batch hop) must match the monolithic engine."""
    import asyncio
    import tempfile, os, threading
    from cake_amd import wire

    cfg_json = dict(
        model_type="llama", hidden_size=128, intermediate_size=256,
        vocab_size=256, num_hidden_layers=4, num_attention_heads=4,
        num_key_value_heads=2, head_dim=32, rms_norm_eps=1e-5,
        rope_theta=10000.0, max_position_embeddings=128,
        tie_word_embeddings=False)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=55)
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        full = cake_amd.Engine(json.dumps(cfg_json), max_seq=64,
                               max_batch_tokens=32,
                               flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
        full.load_safetensors(st)
        lo_eng = cake_amd.Engine(json.dumps(cfg_json), 0, 2, flags=0,
                                 max_seq=64, max_batch_tokens=32)
        lo_eng.load_safetensors(st)
        hi_eng = cake_amd.Engine(json.dumps(cfg_json), 2, 4, flags=0,
                                 max_seq=64, max_batch_tokens=32)
        hi_eng.load_safetensors(st)
        try:
            names = ["model.layers.2", "model.layers.3"]
            worker = wire.WireWorker(hi_eng, names)

            async def run():
                server = await asyncio.start_server(worker.handle,
                                                    "127.0.0.1", 0)
                port = server.sockets[0].getsockname()[1]
                cli = wire.WireClient("127.0.0.1", port)
                await cli.connect()
                assert cli.info["device"] == "gfx950"
                rng = np.random.default_rng(7)
                S = 9
                x = (rng.standard_normal((S, cfg.hidden_size)) * 0.05
                     ).astype(np.float32)
                ref = full.forward_hidden(x, 0)
                a = lo_eng.forward_hidden(x, 0)
                b = await cli.forward_batch(
                    a[None], [(n, 0, 2 + i) for i, n in enumerate(names)])
                assert rel_err(b[0], ref) < 2e-2
                await cli.goodbye()
                server.close()
                await server.wait_closed()

            asyncio.run(asyncio.wait_for(run(), timeout=120))
        finally:
            full.close()
            lo_eng.close()
            hi_eng.close()


def test_gumbel_sampling_semantics():
    """Sampling (text_model.rs:102-118): temp<=0 == greedy; temp>0 is
    seeded-deterministic, seed-sensitive, and samples a different sequence
    than greedy at high temperature."""
    cfg_json = dict(
        model_type="llama", hidden_size=128, intermediate_size=256,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=4,
        num_key_value_heads=2, head_dim=32, max_position_embeddings=256)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=256,
                          max_batch_tokens=64)
    eng.init_random(seed=3)
    try:
        prompt = np.arange(10, dtype=np.uint32)
        greedy = eng.generate_greedy(prompt, 12)
        eng.set_sampling(0.0)
        assert eng.generate_greedy(prompt, 12) == greedy
        eng.set_sampling(5.0, seed=1)
        s1 = eng.generate_greedy(prompt, 12)
        s1b = eng.generate_greedy(prompt, 12)
        assert s1 == s1b, "same seed must reproduce the sample"
        eng.set_sampling(5.0, seed=2)
        s2 = eng.generate_greedy(prompt, 12)
        assert s1 != s2, "different seeds should differ at temp=5"
        assert s1 != greedy, "temp=5 sample should differ from greedy"
        eng.set_sampling(0.0)
        assert eng.generate_greedy(prompt, 12) == greedy
    finally:
        eng.close()


def test_sharded_safetensors_checkpoint():
    """Sharded checkpoints (model.safetensors.index.json + shard files) —
    the layout real HF checkpoints use and cake's VarBuilder reads
    (utils/mod.rs:251-370)."""
    import os, tempfile
    from safetensors.numpy import save_file
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "golden")
    cfg_json, cfg, w, z = fixture_weights(golden, "tiny_llama3")
    tensors = {k: np.ascontiguousarray(v, dtype=np.float32)
               for k, v in flatten(w, cfg).items()}
    with tempfile.TemporaryDirectory() as td:
        # split tensors across two shards + index
        names = sorted(tensors)
        half = len(names) // 2
        shards = {"model-00001-of-00002.safetensors": names[:half],
                  "model-00002-of-00002.safetensors": names[half:]}
        weight_map = {}
        for fn, ns in shards.items():
            save_file({n: tensors[n] for n in ns}, os.path.join(td, fn))
            for n in ns:
                weight_map[n] = fn
        with open(os.path.join(td, "model.safetensors.index.json"),
                  "w") as f:
            json.dump({"metadata": {"total_size": 0},
                       "weight_map": weight_map}, f)

        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=128,
                              max_batch_tokens=64)
        eng.load_safetensors(td)   # directory -> index.json path
        try:
            prompt = z["prompt"].astype(np.uint32)
            _, logits = eng.prefill(prompt, want_logits=True)
            oracle = quantized_oracle(cfg, w)
            ref = oracle.forward(z["prompt"][None, :], 0)[0]
            assert rel_err(logits, ref) < 2e-2
        finally:
            eng.close()
        # missing-tensor error path: an index whose shard list is incomplete
        os.remove(os.path.join(td, "model-00002-of-00002.safetensors"))
        save_file({n: tensors[n] for n in shards[
            "model-00002-of-00002.safetensors"][:-1]},
            os.path.join(td, "model-00002-of-00002.safetensors"))
        e2 = cake_amd.Engine(json.dumps(cfg_json), max_seq=128,
                             max_batch_tokens=64)
        try:
            with pytest.raises(cake_amd.CakeHipError, match="missing"):
                e2.load_safetensors(td)
        finally:
            e2.close()


@pytest.mark.gpu
def test_prefill_graph_replay_matches_eager():
    """The single-chunk pos-0 prefill hipGraph (round 2): first prefill of
    a shape runs eager, the second captures, later ones replay.  All three
    must produce identical logits and greedy ids, and a different prompt
    length afterwards (graph miss -> eager fallback) must still be exact
    vs the oracle-checked decode chain."""
    cfg_json = dict(
        model_type="llama", hidden_size=256, intermediate_size=512,
        vocab_size=512, num_hidden_layers=3, num_attention_heads=4,
        num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-5,
        rope_theta=10000.0, max_position_embeddings=256,
        tie_word_embeddings=False)
    rng = np.random.default_rng(512)
    prompt = rng.integers(0, 512, size=40).astype(np.uint32)
    eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=128,
                          max_batch_tokens=64)
    eng.init_random(seed=7)
    try:
        runs = []
        for _ in range(3):   # eager / capture / replay
            tok, logits = eng.prefill(prompt, want_logits=True)
            ids = [tok] + list(eng.decode(4))
            runs.append((ids, logits.copy()))
            eng.reset()
        for ids, logits in runs[1:]:
            assert ids == runs[0][0], "prefill graph changed greedy ids"
            assert np.array_equal(logits, runs[0][1]), \
                "prefill graph changed logits bit pattern"
        # different length -> graph miss, eager fallback
        p2 = rng.integers(0, 512, size=23).astype(np.uint32)
        t1, l1 = eng.prefill(p2, want_logits=True)
        eng.reset()
        t2, l2 = eng.prefill(p2, want_logits=True)
        assert t1 == t2 and np.array_equal(l1, l2)
    finally:
        eng.close()
