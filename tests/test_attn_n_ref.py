"""CPU half of the head_dim 64 / 96 MFMA prefill attention tests: the
dispatch policy, the variants the op accepts, and the two new configs."""
import os

import numpy as np
import pytest

import cake_amd
from cake_amd.configs import MODELS, SMALL_HEAD_MODELS, find_model

PF_MFMA_N = (1, 4, 0, 0)


def _variant(d):
    return d["pfv"], d["nw"], d["split"], d["deep"]


@pytest.mark.parametrize("hd", [64, 96])
def test_policy_picks_the_mfma_kernel(hd):
    want = (0, 0, 0, 0) if os.environ.get("CAKE_PF_ATTN") == "0" else PF_MFMA_N
    for S in (1, 128, 2048):
        assert _variant(cake_amd.attn_dispatch(S, 14, 2, hd)) == want, S


@pytest.mark.parametrize("hd", [40, 128])
def test_policy_elsewhere_is_the_parents(hd):
    env = lambda k, d: int(os.environ.get(k, d))
    for S in (1, 128, 2048):
        d = cake_amd.attn_dispatch(S, 14, 2, hd)
        nw_env = env("CAKE_PF_NW", 0)
        nw4 = (nw_env == 4) if nw_env else (S + 255) // 256 * 14 < 512
        assert _variant(d) == (env("CAKE_PF_ATTN", 2), 4 if nw4 else 8,
                               int(env("CAKE_PF_SPLIT", 0) != 0),
                               env("CAKE_PF_DEEP", 0)), S
        assert d["split_min_s"] == 1024


@pytest.mark.parametrize("hd,variant", [
    (hd, v) for hd in (64, 96)
    for v in ((1, 8, 0, 0), (1, 4, 1, 0), (2, 4, 0, 0))] + [(40, PF_MFMA_N)])
def test_op_refuses_other_variants_before_any_device_call(hd, variant):
    q = np.zeros((3, 4, hd), np.float32)
    kc = np.zeros((2, 64, hd), np.float32)
    vtc = np.zeros((2, hd, 64), np.float32)
    with pytest.raises(cake_amd.CakeHipError,
                       match=f"op_attn_prefill.*not dispatchable at hd {hd}"):
        cake_amd.op_attn_prefill(q, kc, kc, vtc, 0, 0, variant)


def test_small_head_configs():
    assert set(SMALL_HEAD_MODELS) == {"llama3.2-1b", "phi-3-mini-4k"}
    assert not set(SMALL_HEAD_MODELS) & set(MODELS)
    geom = lambda c: (c["model_type"], c["head_dim"], c["num_attention_heads"],
                      c["num_key_value_heads"], c["hidden_size"],
                      c["intermediate_size"], c["num_hidden_layers"])
    a, b = find_model("llama3.2-1b"), find_model("phi-3-mini-4k")
    assert a is SMALL_HEAD_MODELS["llama3.2-1b"]
    assert geom(a) == ("llama", 64, 32, 8, 2048, 8192, 16)
    assert a["tie_word_embeddings"] is True
    assert a["rope_scaling"]["rope_type"] == "llama3"
    assert geom(b) == ("phi3", 96, 32, 32, 3072, 8192, 32)
    assert b["vocab_size"] == 32064 and not b.get("rope_scaling")
