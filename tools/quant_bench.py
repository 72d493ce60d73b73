#!/usr/bin/env python3
"""Decode tok/s of one configured model under the bench protocol, for
comparing weight formats (bf16 / fp8 / gptq 4-bit) on random-init weights.

Protocol: 128-token seeded prompt, greedy, hipGraph decode, the rate excludes
the first token (it comes from the prefill), two warm runs and three timed
runs of --steps decode steps each.  Prints ONE JSON line; with --stats also
the eager per-kernel kernel_stats() table (us per launch, achieved GB/s over
the algorithmic bytes); with --prefill-len N the prefill rate of an N-token
prompt (two warm passes, one timed).

  python tools/quant_bench.py llama3-8b
  python tools/quant_bench.py llama3-8b-gptq --stats --prefill-len 2048
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 299792458


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", help="a name from MODELS, QUANT_MODELS, "
                    "QWEN2_MODELS, PHI_MODELS, FALCON3_MODELS or "
                    "GEMMA3_MODELS")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--max-seq", type=int, default=4096)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--stats-steps", type=int, default=8)
    ap.add_argument("--prefill-len", type=int, default=0)
    args = ap.parse_args()

    import cake_amd
    from cake_amd.configs import find_model, weight_bytes
    cfg = find_model(args.model)
    flags = cake_amd.HAS_EMBED | cake_amd.HAS_HEAD | cake_amd.USE_GRAPH
    eng = cake_amd.Engine(json.dumps(cfg), flags=flags, max_seq=args.max_seq,
                          max_batch_tokens=2048)
    try:
        eng.init_random(seed=SEED, scale=0.02)
        rng = np.random.default_rng(SEED)
        prompt = rng.integers(0, cfg["vocab_size"],
                              size=args.prompt_len).astype(np.uint32)
        rates = []
        for run in range(5):                   # 2 warm + 3 timed
            eng.reset()
            eng.prefill(prompt)                # token 0: not in the rate
            eng.sync()
            t0 = time.perf_counter()
            toks = eng.decode(args.steps)
            eng.sync()
            dt = time.perf_counter() - t0
            if run >= 2:
                rates.append(args.steps / dt)
        out = {
            "model": args.model, "steps": args.steps,
            "prompt_len": args.prompt_len,
            "decode_tok_s": round(float(np.median(rates)), 2),
            "runs_tok_s": [round(r, 2) for r in rates],
            "weight_gb": round(weight_bytes(cfg) / 1e9, 3),
            "dispatch": cake_amd.decode_dispatch(cfg),
            "last_tokens": [int(t) for t in toks[-4:]],
        }
        if args.prefill_len > 0:
            pf = rng.integers(0, cfg["vocab_size"],
                              size=args.prefill_len).astype(np.uint32)
            for _ in range(2):                 # GEMM plans, then graph capture
                eng.reset()
                eng.prefill(pf)
                eng.sync()
            eng.reset()
            t0 = time.perf_counter()
            eng.prefill(pf)
            eng.sync()
            out["prefill_len"] = args.prefill_len
            out["prefill_tok_s"] = round(
                args.prefill_len / (time.perf_counter() - t0), 1)
        table = None
        if args.stats:
            # eager, per-kernel hipEvent timing
            e2 = cake_amd.Engine(json.dumps(cfg),
                                 flags=cake_amd.HAS_EMBED | cake_amd.HAS_HEAD,
                                 max_seq=args.max_seq, max_batch_tokens=2048)
            try:
                e2.init_random(seed=SEED, scale=0.02)
                e2.prefill(prompt)
                e2.decode(4)
                e2.sync()
                e2.set_stats(True)
                e2.decode(args.stats_steps)
                e2.sync()
                e2.set_stats(False)
                table = e2.kernel_stats()["kernels"]
            finally:
                e2.close()
            out["kernels"] = {
                k: {"launches": v["launches"],
                    "us_per_launch": round(1e3 * v["ms"] / v["launches"], 2),
                    "gb_s": round(v["bytes"] / (v["ms"] * 1e6), 1)
                    if v["ms"] > 0 else None}
                for k, v in table.items()}
        print(json.dumps(out))
        if table:
            print(f"{'kernel':<18}{'launches':>9}{'us/launch':>11}{'GB/s':>9}",
                  file=sys.stderr)
            for k, v in sorted(out["kernels"].items()):
                print(f"{k:<18}{v['launches']:>9}{v['us_per_launch']:>11}"
                      f"{v['gb_s'] or 0:>9}", file=sys.stderr)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
