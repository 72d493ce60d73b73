"""decode_attention "mfma_kv8" (the grouped MFMA decode kernel over the fp8 KV
cache) through the engine (-m gpu), and its host-side plan and refusals (CPU)."""
import numpy as np
import pytest

import cake_amd


def tiny(nh, nkv=1, hd=128, **kw):
    return dict(model_type="llama", hidden_size=256, intermediate_size=512,
                vocab_size=512, num_hidden_layers=2, num_attention_heads=nh,
                num_key_value_heads=nkv, head_dim=hd, rms_norm_eps=1e-5,
                rope_theta=10000.0, max_position_embeddings=512,
                tie_word_embeddings=False, **kw)


# ---- CPU: plan and refusals -------------------------------------------------
@pytest.mark.parametrize("G", [3, 4, 7])
def test_kv_dispatch_group(G):
    cfg = tiny(2 * G, 2, kv_cache_dtype="fp8_e4m3",
               decode_attention="mfma_kv8")
    d = cake_amd.kv_dispatch(cfg, 256)
    assert (d["format"], d["group"], d["grid_y"]) == ("fp8_e4m3", G, 2)


@pytest.mark.parametrize("cfg,kv,keys", [
    (tiny(7), "bf16", ("decode_attention",)),
    (tiny(17), "fp8_e4m3", ("decode_attention",)),
    (tiny(4, hd=64), "fp8_e4m3", ("decode_attention", "kv_cache_dtype"))],
    ids=["bf16-cache", "17-heads", "hd64"])
def test_refusals_name_the_key(cfg, kv, keys):
    full = dict(cfg, kv_cache_dtype=kv, decode_attention="mfma_kv8")
    for call in (lambda: cake_amd.kv_dispatch(full, 64),
                 lambda: cake_amd.Engine(cfg, max_seq=64, kv_dtype=kv,
                                         decode_attention="mfma_kv8")):
        with pytest.raises(cake_amd.CakeHipError, match="|".join(keys)):
            call()


# ---- GPU: G = 3 and 7 on two kv heads, graph replay ---------------------------
PROMPT, GEN, LEG = 250, 12, 6


def engine(nh, mode, flags=None):
    eng = cake_amd.Engine(tiny(nh, 2), max_seq=512, max_batch_tokens=256,
                          flags=flags, kv_dtype="fp8_e4m3",
                          decode_attention=mode)
    eng.init_random(seed=11, scale=0.08)
    return eng


def _split_greedy(eng, prompt):
    """Two decode calls that straddle position 256: the second drops the graph
    captured at 4 chunks, re-zeroes the counters and captures again at 8."""
    first = eng.prefill(prompt)
    return [int(t) for t in
            [first] + list(eng.decode(LEG)) + list(eng.decode(GEN - 1 - LEG))]


@pytest.mark.gpu
@pytest.mark.parametrize("G", [3, 7])
def test_mfma_kv8_vs_default_route(G):
    prompt = np.random.default_rng(5).integers(0, 512, PROMPT).astype(np.uint32)
    new, dflt = engine(2 * G, "mfma_kv8"), engine(2 * G, "auto")
    try:
        ids, want = _split_greedy(new, prompt), _split_greedy(dflt, prompt)
        diff = [i for i in range(GEN) if ids[i] != want[i]]
        if diff:  # a first difference must be a near-tie of the top two
            i = diff[0]
            dflt.reset()
            seq = np.concatenate([prompt, want[:i]]).astype(np.uint32)
            _, lg = dflt.prefill(seq, want_logits=True)
            top = np.argsort(lg)[-2:]
            gap = (lg[top[1]] - lg[top[0]]) / max(1e-9, np.max(np.abs(lg)))
            assert {ids[i], want[i]} == set(int(t) for t in top) and \
                gap < 3e-2, f"token {i}: {ids[i]} vs {want[i]}, gap {gap:.4f}"
    finally:
        new.close()
        dflt.close()


@pytest.mark.gpu
def test_stats_family():
    eng = engine(6, "mfma_kv8", flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD)
    eng.set_stats(True)
    eng.prefill(np.arange(40, dtype=np.uint32))
    eng.decode(2)
    k = eng.kernel_stats()["kernels"]
    eng.close()
    assert k["attn_decode_kv8"]["launches"] == 2 * 2
    assert "attn_decode" not in k
