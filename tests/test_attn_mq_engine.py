"""decode_attention "mfma" (the grouped MFMA decode kernel) through the engine
(-m gpu), and its host-side routing, plan and refusals (CPU)."""
import json
import types

import numpy as np
import pytest

import cake_amd
from oracle import Config, random_weights
from tests import qwen2_ref as qr

# tests/test_qwen2_engine_gpu.py's G = 7 config (hd 128, one kv head)
G7 = dict(
    model_type="qwen2", hidden_size=256, intermediate_size=512,
    vocab_size=512, num_hidden_layers=2, num_attention_heads=7,
    num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-6,
    rope_theta=1000000.0, max_position_embeddings=512,
    tie_word_embeddings=True)


# ---- CPU: routing, plan and refusals ------------------------------------------
def test_routing_is_opt_in(monkeypatch):
    monkeypatch.delenv("CAKE_ATTN_MQ", raising=False)
    assert cake_amd.attn_decode_path(6, 2, 128, 8) == 0
    assert cake_amd.attn_decode_group(4, 2, 64) == 1
    monkeypatch.setenv("CAKE_ATTN_MQ", "1")
    assert cake_amd.attn_decode_path(6, 2, 128, 8) == 4
    assert cake_amd.attn_decode_group(4, 2, 64) == 2
    assert cake_amd.attn_decode_path(6, 2, 96, 8) == 0      # not eligible
    assert cake_amd.attn_decode_path(17, 1, 128, 8) == 0


def test_kv_dispatch_g7(monkeypatch):
    monkeypatch.delenv("CAKE_ATTN_MQ", raising=False)
    cfg = dict(G7, num_attention_heads=14, num_key_value_heads=2)
    assert cake_amd.kv_dispatch(cfg, 256)["group"] == 1
    for c in (cfg, dict(cfg, head_dim=64)):
        d = cake_amd.kv_dispatch(dict(c, decode_attention="mfma"), 256)
        assert (d["group"], d["grid_y"]) == (7, 2)
    assert cake_amd.kv_dispatch(dict(cfg, decode_attention="auto"),
                                256)["group"] == 1


@pytest.mark.parametrize("extra", [
    dict(decode_attention="wmma"),
    dict(decode_attention="mfma", head_dim=96),
    dict(decode_attention="mfma", head_dim=256),
    dict(decode_attention="mfma", num_attention_heads=17),
    dict(decode_attention="mfma", kv_cache_dtype="fp8_e4m3")],
    ids=lambda e: "-".join(map(str, e.values())))
def test_refusals_name_the_key(extra):
    cfg = dict(G7, **extra)
    plain = {k: v for k, v in cfg.items() if k != "decode_attention"}
    for call in (lambda: cake_amd.kv_dispatch(cfg, 64),
                 lambda: cake_amd.Engine(
                     plain, max_seq=64,
                     decode_attention=cfg["decode_attention"])):
        with pytest.raises(cake_amd.CakeHipError, match="decode_attention"):
            call()


# ---- GPU: G = 7 at hd 128 and hd 64, graph replay -----------------------------
PROMPT, GEN, LEG = 250, 12, 6


def _split_greedy(eng, prompt, gen):
    """generate_greedy in two decode calls that straddle position 256.  The
    engine re-reads its chunk-count curve when a decode call begins (and after
    every 64th step of one): the first call replays a graph captured at 4
    chunks (positions 250..255); the second begins at position 256, where the
    grouped curve asks for 8, so it drops the graph, re-zeroes the counters and
    captures again."""
    eng.reset()
    first = eng.prefill(np.asarray(prompt, dtype=np.uint32))
    return ([first] + list(eng.decode(LEG)) + list(eng.decode(gen - 1 - LEG)))


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [128, 64])
def test_g7_mfma_vs_reference(tmp_path, hd):
    """test_hd128_g7_vs_reference's oracle and thresholds, under the default
    flags (graph replay), decoded by _split_greedy so that the chunk count
    changes (4 -> 8) between the two decode calls."""
    from tests.test_gpu_parity import rel_err
    from tests.test_qwen2_engine_gpu import (_greedy_near_tie, _reference,
                                             _write)
    cfg_json = dict(G7, head_dim=hd)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=53)
    biases = qr.random_biases(cfg, seed=54)
    st = str(tmp_path / "m.safetensors")
    _write(w, cfg, biases, st)
    prompt = np.random.default_rng(5).integers(
        0, cfg.vocab_size, size=PROMPT).astype(np.uint32)
    make_ref = lambda: _reference(cfg, w, biases)
    gen, toks = GEN, {}
    for mode in ("mfma", "auto"):
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=512,
                              max_batch_tokens=256, decode_attention=mode)
        try:
            eng.load_safetensors(st)
            split = types.SimpleNamespace(
                generate_greedy=lambda p, g: _split_greedy(eng, p, g))
            if mode == "mfma":
                ref = make_ref().forward(prompt[None, :].astype(np.int64), 0)[0]
                _, logits = eng.prefill(prompt, want_logits=True)
                r = rel_err(logits, ref)
                assert r < 2e-2, f"prefill logits rel err {r}"
                exact = _greedy_near_tie(split, make_ref, list(prompt), gen,
                                         3e-2)
                print(f"qwen2 hd{hd} G7 mfma: {exact}/{gen} greedy ids exact")
            toks[mode] = [int(t) for t in split.generate_greedy(prompt, gen)]
        finally:
            eng.close()
    # against the default kernels on the same weights: equal ids up to a first
    # difference, which must be a near-tie of the reference's top two
    diff = [i for i in range(gen) if toks["mfma"][i] != toks["auto"][i]]
    if diff:
        seq = list(prompt) + toks["auto"][:diff[0]]
        lg = make_ref().forward(np.array([seq], dtype=np.int64), 0)[0]
        srt = np.sort(lg)
        gap = (srt[-1] - srt[-2]) / max(1e-9, np.max(np.abs(lg)))
        assert gap < 3e-2, (f"token {diff[0]}: mfma and auto differ with "
                            f"top-2 gap {gap:.4f}")
