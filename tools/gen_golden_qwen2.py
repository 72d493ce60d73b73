#!/usr/bin/env python3
"""Golden fixture of a tiny qwen2 model: the recipe of oracle/gen_golden.py
for HF transformers' Qwen2ForCausalLM (q/k/v projection bias).

HF initialises the biases to zero, so they are set explicitly: q and k
~ N(0, 3), v ~ N(0, 0.25) from torch.Generator().manual_seed(1), in
named_parameters() order.  The q/k bias is large on purpose: with N(0, 1)
dropping the q bias moves the logits by 1.1e-2 relative and the k bias by
8e-3, both below the engine's 2e-2 gate (a constant added to every key barely
changes a softmax); with N(0, 3) they move by 0.158 / 0.145 / 0.86 (q/k/v).

Asserts, before writing tests/golden/tiny_qwen2.{npz,config.json}:
  logits of tests/qwen2_ref.Qwen2Oracle agree with HF within 2e-4 relative,
  greedy ids are exact,
  zeroing any one of the q, k, v biases moves the reference logits by at
  least 4x the 2e-2 the GPU test grants (tests/test_bias_ref.py re-checks
  this on the committed file).

Run from the repository root:  python tools/gen_golden_qwen2.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import Config  # noqa: E402
from oracle.gen_golden import SEED, flatten_weights, hf_to_oracle  # noqa: E402
from tests import qwen2_ref as qr  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
NAME = "tiny_qwen2"
GPU_GATE = 2e-2          # the engine tests' relative logits limit
DROP_FACTOR = 4.0


def tiny_qwen2_cfg():
    return dict(
        model_type="qwen2", hidden_size=64, intermediate_size=128,
        vocab_size=256, num_hidden_layers=2, num_attention_heads=4,
        num_key_value_heads=2, head_dim=16, rms_norm_eps=1e-6,
        rope_theta=1000000.0, max_position_embeddings=256,
        tie_word_embeddings=True)


def hf_model(cfg_json):
    import torch
    import transformers
    torch.manual_seed(SEED)
    cfg = transformers.Qwen2Config(
        hidden_size=cfg_json["hidden_size"],
        intermediate_size=cfg_json["intermediate_size"],
        vocab_size=cfg_json["vocab_size"],
        num_hidden_layers=cfg_json["num_hidden_layers"],
        num_attention_heads=cfg_json["num_attention_heads"],
        num_key_value_heads=cfg_json["num_key_value_heads"],
        rms_norm_eps=cfg_json["rms_norm_eps"],
        rope_theta=cfg_json["rope_theta"],
        max_position_embeddings=cfg_json["max_position_embeddings"],
        tie_word_embeddings=cfg_json["tie_word_embeddings"],
        use_sliding_window=False)
    m = transformers.Qwen2ForCausalLM(cfg).eval().float()
    assert m.config.hidden_size // m.config.num_attention_heads == \
        cfg_json["head_dim"]
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(("q_proj.bias", "k_proj.bias")):
                p.copy_(torch.randn(p.shape, generator=g) * 3.0)
            elif name.endswith("v_proj.bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.25)
    return m


def drop_one_moves(cfg, w, biases, prompt, logits):
    """{q|k|v: relative move of the reference logits with that bias zeroed}."""
    out = {}
    for which in "qkv":
        o = qr.Qwen2Oracle(cfg, w, qr.drop_one(biases, cfg, which))
        lg = o.forward(prompt[None, :], 0)[0]
        out[which] = float(np.max(np.abs(lg - logits)) /
                           np.max(np.abs(logits)))
    return out


def main(prompt_len=17, gen=12):
    import torch
    cfg_json = tiny_qwen2_cfg()
    m = hf_model(cfg_json)
    cfg = Config.from_json(cfg_json)
    w = hf_to_oracle(m, cfg)
    sd = {k: v.detach().numpy().astype(np.float32)
          for k, v in m.state_dict().items()}
    biases = qr.fused_biases(sd, cfg)
    oracle = qr.Qwen2Oracle(cfg, w, biases)

    rng = np.random.default_rng(SEED)
    prompt = rng.integers(0, cfg.vocab_size, size=prompt_len).astype(np.int64)
    with torch.no_grad():
        hf_logits = m(torch.tensor(prompt[None, :])).logits[0, -1].numpy()
        hf_gen = m.generate(torch.tensor(prompt[None, :]), max_new_tokens=gen,
                            do_sample=False, use_cache=True,
                            pad_token_id=0)[0, prompt_len:].numpy()
    or_logits = oracle.forward(prompt[None, :], 0)[0]
    oracle.reset()
    or_gen = np.array(oracle.generate_greedy(list(prompt), gen))
    rel = np.max(np.abs(hf_logits - or_logits)) / np.max(np.abs(hf_logits))
    print(f"[{NAME}] logits rel diff vs HF = {rel:.3e}; greedy exact = "
          f"{np.array_equal(hf_gen, or_gen)}")
    assert rel < 2e-4, "the qwen2 reference does not match HF transformers"
    assert np.array_equal(hf_gen, or_gen), "greedy ids differ from HF"
    moves = drop_one_moves(cfg, w, biases, prompt, or_logits)
    print(f"[{NAME}] drop-one moves of the logits: {moves}")
    assert min(moves.values()) >= DROP_FACTOR * GPU_GATE, moves

    arrs = {"w." + k: v for k, v in flatten_weights(w, cfg).items()}
    arrs.update({"w." + k: v
                 for k, v in qr.bias_tensors(biases, cfg).items()})
    arrs.update(prompt=prompt, hf_logits=hf_logits, hf_gen=hf_gen,
                oracle_logits=or_logits)
    np.savez_compressed(os.path.join(GOLDEN_DIR, f"{NAME}.npz"), **arrs)
    with open(os.path.join(GOLDEN_DIR, f"{NAME}.config.json"), "w") as f:
        json.dump(cfg_json, f, indent=1)
    print(f"[{NAME}] fixture written to tests/golden/{NAME}.npz")


if __name__ == "__main__":
    main()
