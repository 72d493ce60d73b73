"""The fp8 (e4m3) KV cache through the engine (-m gpu), and its host-side plan
and refusals (CPU)."""
import numpy as np
import pytest

import cake_amd
from oracle import Config, OracleModel, random_weights
from tests.helpers import weights_to_safetensors

LLAMA3_8B = dict(model_type="llama", hidden_size=4096, intermediate_size=14336,
                 vocab_size=128256, num_hidden_layers=32,
                 num_attention_heads=32, num_key_value_heads=8,
                 max_position_embeddings=8192)


def tiny(nh, hd=128, **kw):
    return dict(model_type="llama", hidden_size=256, intermediate_size=512,
                vocab_size=512, num_hidden_layers=2, num_attention_heads=nh,
                num_key_value_heads=1, head_dim=hd, rms_norm_eps=1e-5,
                rope_theta=10000.0, max_position_embeddings=128,
                tie_word_embeddings=False, **kw)


# ---- CPU: plan and refusals -------------------------------------------------
def test_kv_dispatch_bytes_llama3_8b():
    rows, elems = 8 * 8192, 8 * 8192 * 128
    bf = cake_amd.kv_dispatch(LLAMA3_8B, 8192)
    f8 = cake_amd.kv_dispatch(dict(LLAMA3_8B, kv_cache_dtype="fp8_e4m3"), 8192)
    assert bf == dict(format="bf16", layer_bytes=6 * elems, scratch_bytes=0,
                      group=4, grid_y=8)
    assert f8 == dict(format="fp8_e4m3", layer_bytes=2 * elems + 8 * rows,
                      scratch_bytes=6 * elems, group=4, grid_y=8)
    assert cake_amd.kv_dispatch(dict(LLAMA3_8B, kv_cache_dtype="bf16"),
                                8192) == bf
    assert cake_amd.kv_dispatch(dict(tiny(3), kv_cache_dtype="fp8_e4m3"),
                                64)["grid_y"] == 3


@pytest.mark.parametrize("hd", [64, 256])
def test_fp8_kv_refuses_other_head_dims(hd):
    cfg = dict(tiny(4, hd), kv_cache_dtype="fp8_e4m3")
    for call in (lambda: cake_amd.kv_dispatch(cfg, 64),
                 lambda: cake_amd.Engine(tiny(4, hd), max_seq=64,
                                         kv_dtype="fp8_e4m3")):
        with pytest.raises(cake_amd.CakeHipError) as ei:
            call()
        assert "kv_cache_dtype" in str(ei.value) and str(hd) in str(ei.value)


def test_unknown_kv_dtype_refused():
    with pytest.raises(cake_amd.CakeHipError, match="kv_cache_dtype"):
        cake_amd.kv_dispatch(dict(tiny(4), kv_cache_dtype="int8"), 64)


# ---- GPU: the engine --------------------------------------------------------
EAGER = cake_amd.HAS_EMBED | cake_amd.HAS_HEAD


def engine(nh, kv_dtype, flags=None, bt=64):
    eng = cake_amd.Engine(tiny(nh), max_seq=64, max_batch_tokens=bt,
                          flags=flags, kv_dtype=kv_dtype)
    eng.init_random(seed=11, scale=0.08)
    return eng


def prompt(n=40):
    return np.random.default_rng(5).integers(0, 512, n).astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("nh", [4, 3])
def test_prefill_logits_vs_oracle(nh, tmp_path):
    """Both cache formats against the float64 oracle.  Measured on MI355X
    (max |d logits| / max |logits|): see DESIGN section 2.  The fp8 engine may
    add the e4m3 half-ulp, 2^-4 relative per K / V element, which the softmax
    and the two-layer stack average down; the gate is the smoke gate 5e-2."""
    cfg = Config.from_json(tiny(nh))
    w = random_weights(cfg, seed=7)
    ref = OracleModel(cfg, w).forward(prompt()[None, :].astype(np.int64), 0)[0]
    st = str(tmp_path / "m.safetensors")
    weights_to_safetensors(w, cfg, st)
    rel = {}
    for kv in ("bf16", "fp8_e4m3"):
        eng = cake_amd.Engine(tiny(nh), max_seq=64, max_batch_tokens=64,
                              kv_dtype=kv)
        eng.load_safetensors(st)
        _, logits = eng.prefill(prompt(), want_logits=True)
        eng.close()
        rel[kv] = np.max(np.abs(logits - ref)) / np.max(np.abs(ref))
    print(f"G={nh}: rel err vs oracle bf16 {rel['bf16']:.3e} "
          f"fp8 {rel['fp8_e4m3']:.3e}")
    assert rel["bf16"] < 5e-2 and rel["fp8_e4m3"] < 5e-2


@pytest.mark.gpu
@pytest.mark.parametrize("nh", [4, 3])
def test_routes_agree_exactly(nh):
    """Prefill (bf16 scratch) and decode (codes) attend to identical values,
    so chunking, graph replay and reset change no greedy id."""
    whole = engine(nh, "fp8_e4m3", flags=EAGER)
    first = whole.prefill(prompt())
    ids = [first] + list(whole.decode(12))
    chunked = engine(nh, "fp8_e4m3", flags=EAGER, bt=16)
    assert [chunked.prefill(prompt())] + list(chunked.decode(12)) == ids
    graph = engine(nh, "fp8_e4m3")
    assert [graph.prefill(prompt())] + list(graph.decode(12)) == ids
    whole.reset()
    assert [whole.prefill(prompt())] + list(whole.decode(12)) == ids
    # cached decode against the uncached forward (the bf16 engines' bound)
    seq = np.concatenate([prompt(), ids[:3]]).astype(np.uint32)
    whole.reset()
    _, logits = whole.prefill(seq, want_logits=True)
    assert int(np.argmax(logits)) == ids[3]
    for e in (whole, chunked, graph):
        e.close()


@pytest.mark.gpu
def test_stats_families():
    eng = engine(4, "fp8_e4m3", flags=EAGER, bt=16)
    eng.set_stats(True)
    eng.prefill(prompt())
    eng.decode(2)
    k = eng.kernel_stats()["kernels"]
    assert k["kv8_quant"]["launches"] == 2 * 3 + 2 * 2
    assert k["kv8_dequant"]["launches"] == 2 * 2
    assert k["attn_decode_kv8"]["launches"] == 2 * 2
    assert "attn_decode" not in k
    eng.close()
