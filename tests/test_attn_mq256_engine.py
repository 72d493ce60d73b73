"""decode_attention "mfma_256" (k_attn_decode_mq256) through the engine
(-m gpu), and its host-side routing, plan and refusals (CPU)."""
import json
import types

import numpy as np
import pytest

import cake_amd
from oracle import Config
from tests.test_attn_mq_engine import GEN, PROMPT, _split_greedy
from tests.test_falcon3_engine_gpu import (SMALL, _greedy_near_tie, _model,
                                           rel_err)

G3 = SMALL["g3"]                                 # llama, hd 256, 6 / 2 heads


def test_routing_is_opt_in(monkeypatch):
    for knob in ("CAKE_ATTN_MQ", "CAKE_ATTN_MQ256", "CAKE_ATTN256_GB"):
        monkeypatch.delenv(knob, raising=False)
    assert cake_amd.attn_decode_path(6, 2, 256, 8) == 3
    assert cake_amd.attn_decode_group(6, 2, 256) == 1
    monkeypatch.setenv("CAKE_ATTN_MQ", "1")                  # not this knob
    assert cake_amd.attn_decode_path(6, 2, 256, 8) == 3
    monkeypatch.delenv("CAKE_ATTN_MQ")
    monkeypatch.setenv("CAKE_ATTN_MQ256", "1")
    assert cake_amd.attn_decode_path(6, 2, 256, 8) == 5
    assert cake_amd.attn_decode_group(6, 2, 256) == 3
    assert cake_amd.attn_decode_path(17, 1, 256, 8) == 3     # not eligible
    assert cake_amd.attn_decode_path(6, 2, 128, 8) == 0      # hd 256 only


def test_kv_dispatch(monkeypatch):
    for knob in ("CAKE_ATTN_MQ256", "CAKE_ATTN256_GB"):
        monkeypatch.delenv(knob, raising=False)
    assert cake_amd.kv_dispatch(G3, 256)["group"] == 1
    for nh, nkv in ((6, 2), (4, 1), (16, 1)):
        d = cake_amd.kv_dispatch(dict(G3, num_attention_heads=nh,
                                      num_key_value_heads=nkv,
                                      decode_attention="mfma_256"), 256)
        assert (d["group"], d["grid_y"]) == (nh // nkv, nkv)


@pytest.mark.parametrize("extra", [  # head dim 128; 17 heads per kv head
    dict(head_dim=128), dict(num_attention_heads=17, num_key_value_heads=1)])
def test_refusals_name_the_key(extra):
    plain = dict(G3, **extra)
    for call in (lambda: cake_amd.kv_dispatch(
                     dict(plain, decode_attention="mfma_256"), 64),
                 lambda: cake_amd.Engine(plain, max_seq=64,
                                         decode_attention="mfma_256")):
        with pytest.raises(cake_amd.CakeHipError, match="decode_attention"):
            call()


@pytest.mark.gpu
@pytest.mark.parametrize("name,prompt_len", [
    ("g3", 40), ("g4", 40), ("mistral-window16", 40), ("g3", PROMPT)])
def test_mfma_256_vs_oracle(tmp_path, name, prompt_len):
    """test_small_config_vs_oracle's configs, oracle and gates under "mfma_256"
    and graph replay, then the ids against the "auto" engine.  The 250-token
    prompt is decoded across the chunk-count change (4 -> 8) at position 256."""
    cfg_json, st = SMALL[name], str(tmp_path / "m.safetensors")
    cfg = Config.from_json(cfg_json)
    make_ref, gate = _model(name, cfg_json, cfg, st)
    prompt = np.random.default_rng(5).integers(
        0, cfg.vocab_size, size=prompt_len).astype(np.uint32)
    gen, toks = (GEN if prompt_len == PROMPT else 6), {}
    for mode in ("mfma_256", "auto"):
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=512,
                              max_batch_tokens=256, decode_attention=mode)
        try:
            eng.load_safetensors(st)
            run = eng if prompt_len != PROMPT else types.SimpleNamespace(
                generate_greedy=lambda p, g: _split_greedy(eng, p, g))
            if mode == "mfma_256":
                ref = make_ref().forward(prompt[None, :].astype(np.int64), 0)[0]
                _, logits = eng.prefill(prompt, want_logits=True)
                assert rel_err(logits, ref) < gate, "prefill logits"
                _greedy_near_tie(run, make_ref, list(prompt), gen, 3e-2)
            toks[mode] = [int(t) for t in run.generate_greedy(prompt, gen)]
        finally:
            eng.close()
    # equal ids up to a first difference: a near-tie of the reference's top two
    diff = [i for i in range(gen) if toks["mfma_256"][i] != toks["auto"][i]]
    if diff:
        seq = list(prompt) + toks["auto"][:diff[0]]
        lg = make_ref().forward(np.array([seq], dtype=np.int64), 0)[0]
        srt = np.sort(lg)
        gap = (srt[-1] - srt[-2]) / max(1e-9, np.max(np.abs(lg)))
        assert gap < 3e-2, (f"token {diff[0]}: mfma_256 and auto differ with "
                            f"top-2 gap {gap:.4f}")
