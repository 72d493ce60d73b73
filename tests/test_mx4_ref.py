"""CPU tests of the MXFP4 path: the reference's code table and nibble order,
the config refusals of engine create (no device call is made before the config
is accepted), the model table and the byte accounting."""
import json

import numpy as np
import pytest

import cake_amd
from cake_amd.configs import LLAMA3_8B, find_model, weight_bytes
from tests import mx4_ref as mr

TINY = dict(model_type="llama", hidden_size=256, intermediate_size=512,
            vocab_size=512, num_hidden_layers=2, num_attention_heads=2,
            num_key_value_heads=1, head_dim=128, max_position_embeddings=512)
WEIGHT = dict(dtype="fp4", qscheme="per_group", group_size=32, ch_axis=-1,
              scale_format="e8m0")


def quark(model=TINY, top={}, **w):
    return dict(model, quantization_config=dict(
        quant_method="quark",
        global_quant_config=dict(weight=dict(WEIGHT, **w)), **top))


def test_dequant_of_the_sixteen_codes_and_nibble_order():
    w, s = mr.pack(np.tile(np.arange(16), 2)[None], [[128]])    # scale 2
    assert w[0, 0] == 0x10 and w[0, 7] == 0xFE              # low nibble first
    mag = [0, 1, 2, 3, 4, 6, 8, 12]
    assert list(mr.dequant(w, s)[0, :16]) == mag + [-m for m in mag]
    assert np.signbit(mr.dequant(w, s)[0, 8])               # code 8 is -0


@pytest.mark.parametrize("cfg,msg", [
    (quark(group_size=64), r"group_size 64"),
    (quark(dtype="fp6_e2m3"), r"dtype fp6_e2m3"),
    (quark(scale_format="float16"), r"scale_format float16"),
    (quark(qscheme="per_channel"), r"qscheme per_channel"),
    (quark(top=dict(layer_quant_config={"*down_proj": {}})),
     r"layer_quant_config"),
    (quark(dict(TINY, model_type="gemma3_text")),
     r"quark with model_type gemma3.*GELU"),
    (quark(dict(TINY, hidden_size=272)), r"in_features 272"),
], ids=["group64", "dtype", "scale_format", "qscheme", "layer_config",
        "gemma3", "k_not_32"])
def test_config_refusals_name_the_field(cfg, msg):
    with pytest.raises(cake_amd.CakeHipError, match=msg):
        cake_amd.Engine(json.dumps(cfg), max_seq=64, max_batch_tokens=32)


def test_models_dispatch_and_bytes():
    c = find_model("llama3-8b-mxfp4")
    d = cake_amd.decode_dispatch(c)
    assert d["qkv"] == ("gemv_mx4", 4, 1) and d["down"] == ("gemv_mx4", 4, 4)
    assert d["gateup"] == ("gateup_mx4", 4, 1) and "mx4" not in d["head"][0]
    # 17/32 bytes per weight in the projections, the rest as bf16
    n = 32 * (6144 * 4096 + 4096 * 4096 + 3 * 14336 * 4096)
    assert weight_bytes(LLAMA3_8B) - weight_bytes(c) == n * 2 - n * 17 // 32
