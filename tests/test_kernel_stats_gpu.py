"""GPU test (-m gpu) of the engine's kernel_stats() bookkeeping: for five
small configs (every decode route and weight format) the table {family:
(launches, bytes, flops)} of one prefill and three eager decode steps equals
tests/golden/kernel_stats_families.json, recorded by
tools/record_kernel_stats.py.  The quantities are integers below 2^53 and
compare exactly; ms is not compared."""
import json
import os

import numpy as np
import pytest

import cake_amd

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "kernel_stats_families.json")
BASE = dict(
    hidden_size=256, intermediate_size=512, vocab_size=512,
    num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
    head_dim=64, rms_norm_eps=1e-5, rope_theta=10000.0,
    max_position_embeddings=128, tie_word_embeddings=False)
CONFIGS = {
    # fused norm -> qkv GEMV -> rope -> KV-store decode kernel
    "llama_bf16": dict(BASE, model_type="llama"),
    # QK-norm: GEMV, then rope_store
    "qwen3_bf16": dict(BASE, model_type="qwen3"),
    # the biased fused kernel
    "qwen2_bf16": dict(BASE, model_type="qwen2"),
    # every dimension is a multiple of 128 (Sq 256, Skv 128)
    "llama_fp8": dict(BASE, model_type="llama",
                      quantization_config=dict(quant_method="fp8")),
    "llama_gptq": dict(BASE, model_type="llama",
                       quantization_config=dict(quant_method="gptq", bits=4,
                                                group_size=32,
                                                desc_act=False)),
}
PROMPT = np.array([3, 141, 59, 265, 358], dtype=np.uint32)
DECODE_STEPS = 3
SEED = 1234


def stats_table(cfg_json):
    """{family: [launches, bytes, flops]} of prefill(5 tokens) + 3 decode
    steps, stats on, graphs off, init_random weights."""
    eng = cake_amd.Engine(json.dumps(cfg_json),
                          flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD,
                          max_seq=64, max_batch_tokens=32)
    try:
        eng.init_random(seed=SEED)
        eng.set_stats(True)
        eng.prefill(PROMPT)
        eng.decode(DECODE_STEPS)
        eng.sync()
        eng.set_stats(False)
        st = eng.kernel_stats()
    finally:
        eng.close()
    assert not st["truncated"]
    return {k: [v["launches"], v["bytes"], v["flops"]]
            for k, v in sorted(st["kernels"].items())}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_configs(golden):
    assert sorted(golden) == sorted(CONFIGS)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_kernel_stats_families(name, golden):
    got = stats_table(CONFIGS[name])
    want = golden[name]
    for fam in sorted(set(got) | set(want)):
        print(name, fam, "got", got.get(fam), "want", want.get(fam))
    assert got == want
