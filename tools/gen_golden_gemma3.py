#!/usr/bin/env python3
"""Golden fixture of a tiny Gemma 3 text model: HF transformers'
Gemma3ForCausalLM on the CPU (head_dim 256 with nh 2, nkv 1; H 32, I 16, V 48;
three layers sliding, full, sliding with window 8; query_pre_attn_scalar 128;
the global rope linear with factor 4 at theta 1e6, the local one at theta 1e4),
the recipe of tools/gen_golden_falcon3.py.

HF initialises every norm weight to 0; here they are drawn (sigma 0.1) so that
w and 1 + w differ visibly.  QK-norm cancels any scaling of the q and k
projection rows, so attention is sharpened through the q_norm / k_norm weights
instead: 1 + w = s (1 + 0.1 n), with s the smallest of SCALES at which every
defect of tests/gemma3_ref.DEFECTS moves the reference logits by at least 4x
the engine tests' 2e-2 gate, while the bf16-activation estimate stays within
half the gate of HF.  The gate_proj rows are scaled by GATE_SCALE: at HF's
initializer range the gate pre-activations are of order 0.1, where SiLU and
GELU-tanh are both g / 2 to first order and a wrong gate would not show.  The
embedding rows are scaled by EMBED_SCALE: the post norms make every branch
output of rms ~1, and beside them HF's initial rows (rms 0.11 after the
sqrt(H) scale) would leave a residual stream made of rounding-sensitive branch
outputs alone, which a model this narrow (H 32) does not average out.

All weights are rounded to bf16-representable values BEFORE HF runs.  Asserts,
before writing tests/golden/tiny_gemma3.{npz,config.json}: the reference agrees
with HF within 2e-4 relative on the 17-token prompt, the 12 greedy ids are
exact, the defect and headroom conditions above, and the file is no larger than
its biggest sibling.

Run from the repository root:  python tools/gen_golden_gemma3.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import SEED  # noqa: E402
from tests import gemma3_ref as gr  # noqa: E402
from tests.helpers import quantize_bf16  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
NAME = "tiny_gemma3"
GPU_GATE = 2e-2          # the engine tests' relative logits limit
DEFECT_FACTOR = 4.0
MAX_SEQ = 64
SCALES = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)
GATE_SCALE = 8.0         # gate pre-activations of order 1, see above
EMBED_SCALE = 8.0        # scaled embedding rows of rms ~1, see above


def tiny_gemma3_cfg():
    return dict(
        model_type="gemma3_text", hidden_size=32, intermediate_size=16,
        vocab_size=48, num_hidden_layers=3, num_attention_heads=2,
        num_key_value_heads=1, head_dim=256, rms_norm_eps=1e-6,
        max_position_embeddings=256, sliding_window=8,
        query_pre_attn_scalar=128, hidden_activation="gelu_pytorch_tanh",
        layer_types=["sliding_attention", "full_attention",
                     "sliding_attention"],
        rope_parameters=dict(
            full_attention=dict(rope_type="linear", factor=4.0,
                                rope_theta=1000000.0),
            sliding_attention=dict(rope_type="default", rope_theta=10000.0)),
        final_logit_softcapping=None, attn_logit_softcapping=None,
        tie_word_embeddings=True)


def hf_model(cfg_json, qk_scale):
    import torch
    import transformers
    torch.manual_seed(SEED)
    kw = {k: v for k, v in cfg_json.items() if k != "model_type"}
    cfg = transformers.Gemma3TextConfig(
        **kw, pad_token_id=0, bos_token_id=1, eos_token_id=None,
        attn_implementation="eager")
    m = transformers.Gemma3ForCausalLM(cfg).eval().float()
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(("q_norm.weight", "k_norm.weight")):
                p.copy_(float(qk_scale) *
                        (1 + 0.1 * torch.randn(p.shape, generator=g)) - 1)
            elif name.endswith("norm.weight"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("gate_proj.weight"):
                p *= GATE_SCALE
            elif name.endswith("embed_tokens.weight"):
                p *= EMBED_SCALE
            p.copy_(torch.from_numpy(quantize_bf16(p.numpy())))
    return m


def evaluate(qk_scale, prompt, gen):
    import torch
    cfg_json = tiny_gemma3_cfg()
    m = hf_model(cfg_json, qk_scale)
    t = {k: v.detach().numpy().astype(np.float32)
         for k, v in m.state_dict().items() if k != "lm_head.weight"}
    with torch.no_grad():
        hf_logits = m(torch.tensor(prompt[None, :])).logits[0, -1].numpy()
        hf_gen = m.generate(torch.tensor(prompt[None, :]), max_new_tokens=gen,
                            do_sample=False, use_cache=True,
                            pad_token_id=0)[0, len(prompt):].numpy()
    moves, lg = gr.defect_moves(cfg_json, t, prompt, MAX_SEQ)
    est = gr.Gemma3Oracle(cfg_json, t, MAX_SEQ, act_bf16=True).forward(
        prompt[None, :], 0)[0]
    or_gen = np.array(gr.Gemma3Oracle(cfg_json, t, MAX_SEQ).generate_greedy(
        list(prompt), gen))
    return dict(cfg_json=cfg_json, t=t, hf_logits=hf_logits, hf_gen=hf_gen,
                or_gen=or_gen, rel=gr.rel(lg, hf_logits), moves=moves,
                headroom=gr.rel(est, hf_logits))


def main(prompt_len=17, gen=12):
    rng = np.random.default_rng(SEED)
    prompt = rng.integers(0, tiny_gemma3_cfg()["vocab_size"],
                          size=prompt_len).astype(np.int64)
    need = DEFECT_FACTOR * GPU_GATE
    chosen = None
    for scale in SCALES:
        r = evaluate(scale, prompt, gen)
        print(f"[{NAME}] q/k norm x{scale}: moves "
              f"{ {k: round(v, 4) for k, v in r['moves'].items()} } "
              f"bf16-activation estimate vs HF {r['headroom']:.3e}")
        if min(r["moves"].values()) >= need and \
                r["headroom"] <= GPU_GATE / 2:
            chosen = (scale, r)
            break
    assert chosen, "no scale meets the defect and headroom conditions"
    scale, r = chosen
    print(f"[{NAME}] chosen: q/k norm x{scale}; logits rel diff vs HF "
          f"{r['rel']:.3e}; greedy exact = "
          f"{np.array_equal(r['hf_gen'], r['or_gen'])}")
    assert r["rel"] < 2e-4, "the reference does not match HF transformers"
    assert np.array_equal(r["hf_gen"], r["or_gen"]), "greedy ids differ from HF"
    assert r["headroom"] <= GPU_GATE / 2, r["headroom"]

    arrs = {"w." + k: v for k, v in r["t"].items()}
    arrs.update(prompt=prompt, hf_logits=r["hf_logits"], hf_gen=r["hf_gen"],
                qk_scale=np.float64(scale))
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
    assert size <= biggest, "shrink H, I and V first"


if __name__ == "__main__":
    main()
