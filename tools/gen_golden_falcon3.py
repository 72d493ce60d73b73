#!/usr/bin/env python3
"""Golden fixture of a tiny Falcon3-shaped model: HF transformers'
LlamaForCausalLM with head_dim 256 (nh 2, nkv 1: G = 2, H 64, I 8, V 48, 2
layers; I and V are that small to keep the file under its siblings' size), the
recipe of tools/gen_golden_phi3.py.

An ordinary random model does not show a wrong attention at the engine tests'
2e-2 logits gate (near-uniform softmax: the output is the mean of V whatever
the scores are), so the q and k rows of every layer are scaled by the smallest
power of two at which each defect of tests/falcon3_ref.ATTN_DEFECTS (score over
dims [0, 128) only; output dims [128, 256) taken from [0, 128); scale
1/sqrt(128)) moves the reference logits by at least 4x the gate, while the
bf16-activation estimate stays within half the gate of HF.

All weights are rounded to bf16-representable values BEFORE HF runs.  Asserts,
before writing tests/golden/tiny_falcon3.{npz,config.json}: the reference
agrees with HF within 2e-4 relative on the 17-token prompt, the 12 greedy ids
are exact, the defect and headroom conditions above, and the file is no larger
than its biggest sibling.

Run from the repository root:  python tools/gen_golden_falcon3.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import Config  # noqa: E402
from oracle.gen_golden import SEED, flatten_weights, hf_to_oracle  # noqa: E402
from tests import falcon3_ref as fr  # noqa: E402
from tests.helpers import quantize_bf16  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
NAME = "tiny_falcon3"
GPU_GATE = 2e-2          # the engine tests' relative logits limit
DEFECT_FACTOR = 4.0
MAX_SEQ = 64
SCALES = (1, 2, 4, 8, 16, 32, 64)


def tiny_falcon3_cfg():
    return dict(
        model_type="llama", hidden_size=64, intermediate_size=8,
        vocab_size=48, num_hidden_layers=2, num_attention_heads=2,
        num_key_value_heads=1, head_dim=256, rms_norm_eps=1e-6,
        rope_theta=1000042.0, max_position_embeddings=256,
        tie_word_embeddings=False)


def hf_model(cfg_json, qk_scale):
    import torch
    import transformers
    torch.manual_seed(SEED)
    cfg = transformers.LlamaConfig(
        hidden_size=cfg_json["hidden_size"],
        intermediate_size=cfg_json["intermediate_size"],
        vocab_size=cfg_json["vocab_size"],
        num_hidden_layers=cfg_json["num_hidden_layers"],
        num_attention_heads=cfg_json["num_attention_heads"],
        num_key_value_heads=cfg_json["num_key_value_heads"],
        head_dim=cfg_json["head_dim"],
        rms_norm_eps=cfg_json["rms_norm_eps"],
        rope_theta=cfg_json["rope_theta"],
        max_position_embeddings=cfg_json["max_position_embeddings"],
        tie_word_embeddings=False, attention_bias=False, mlp_bias=False,
        pad_token_id=0, bos_token_id=1, eos_token_id=None,  # never stop early
        attn_implementation="eager")
    m = transformers.LlamaForCausalLM(cfg).eval().float()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(("q_proj.weight", "k_proj.weight")):
                p *= float(qk_scale)
            p.copy_(torch.from_numpy(quantize_bf16(p.numpy())))
    return m


def evaluate(qk_scale, prompt, gen):
    import torch
    cfg_json = tiny_falcon3_cfg()
    m = hf_model(cfg_json, qk_scale)
    cfg = Config.from_json(cfg_json)
    w = hf_to_oracle(m, cfg)
    with torch.no_grad():
        hf_logits = m(torch.tensor(prompt[None, :])).logits[0, -1].numpy()
        hf_gen = m.generate(torch.tensor(prompt[None, :]), max_new_tokens=gen,
                            do_sample=False, use_cache=True,
                            pad_token_id=0)[0, len(prompt):].numpy()
    moves, lg = fr.defect_moves(cfg, w, cfg_json, prompt, MAX_SEQ)
    est = fr.Hd256Oracle(cfg, w, cfg_json, MAX_SEQ, act_bf16=True).forward(
        prompt[None, :], 0)[0]
    o = fr.Hd256Oracle(cfg, w, cfg_json, MAX_SEQ)
    or_gen = np.array(o.generate_greedy(list(prompt), gen))
    return dict(cfg_json=cfg_json, cfg=cfg, w=w, hf_logits=hf_logits,
                hf_gen=hf_gen, or_gen=or_gen, rel=fr.rel(lg, hf_logits),
                moves=moves, headroom=fr.rel(est, hf_logits))


def main(prompt_len=17, gen=12):
    rng = np.random.default_rng(SEED)
    prompt = rng.integers(0, tiny_falcon3_cfg()["vocab_size"],
                          size=prompt_len).astype(np.int64)
    need = DEFECT_FACTOR * GPU_GATE
    chosen = None
    for scale in SCALES:
        r = evaluate(scale, prompt, gen)
        print(f"[{NAME}] q/k rows x{scale}: moves "
              f"{ {k: round(v, 4) for k, v in r['moves'].items()} } "
              f"bf16-activation estimate vs HF {r['headroom']:.3e}")
        if min(r["moves"].values()) >= need:
            chosen = (scale, r)
            break
    assert chosen, "no scale meets the defect condition"
    scale, r = chosen
    print(f"[{NAME}] chosen: q/k rows x{scale}; logits rel diff vs HF "
          f"{r['rel']:.3e}; greedy exact = "
          f"{np.array_equal(r['hf_gen'], r['or_gen'])}")
    assert r["rel"] < 2e-4, "the reference does not match HF transformers"
    assert np.array_equal(r["hf_gen"], r["or_gen"]), "greedy ids differ from HF"
    assert r["headroom"] <= GPU_GATE / 2, r["headroom"]

    arrs = {"w." + k: v for k, v in flatten_weights(r["w"], r["cfg"]).items()}
    arrs.update(prompt=prompt, hf_logits=r["hf_logits"], hf_gen=r["hf_gen"],
                qk_scale=np.int64(scale))
    path = os.path.join(GOLDEN_DIR, f"{NAME}.npz")
    np.savez_compressed(path, **arrs)
    with open(os.path.join(GOLDEN_DIR, f"{NAME}.config.json"), "w") as f:
        json.dump(r["cfg_json"], f, indent=1)
    size = os.path.getsize(path)
    biggest = max(os.path.getsize(os.path.join(GOLDEN_DIR, n))
                  for n in os.listdir(GOLDEN_DIR)
                  if n.endswith(".npz") and n != f"{NAME}.npz")
    print(f"[{NAME}] fixture written to tests/golden/{NAME}.npz "
          f"({size} bytes; biggest sibling {biggest})")
    assert size <= biggest, "shrink I and V first"


if __name__ == "__main__":
    main()
