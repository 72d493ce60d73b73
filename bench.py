#!/usr/bin/env python3
"""Benchmark — cake's headline metric (decode tok/s + prefill tok/s) on the
MI355X-native engine, per BASELINE.json.

Contract: `python bench.py --gpus N --steps K --warmup W`; for N>1 launched
by torchrun with one rank per GPU; rank 0 prints ONE JSON line.  A plain run
does only what the headline figure needs: set up, prefill the prompt, warm
up, time K decode steps, print.  `--full` adds every other leg (per-kernel
roofline stats, prefill rate, CPU baseline, the model matrix); without it
those keys of the JSON line are null.  `--dump-outputs DIR` writes what the
timed decode call returned (the K greedy token ids) as DIR/tokens.npy.
A "step" is
one greedy KV-cached decode token (the reference's per-token hot loop,
text_model.rs:397-495; rate convention excludes the first token like
master.rs:131-166).  N>1 = the model layer-sharded as contiguous pipeline
ranges with the activation hop over RCCL/xGMI (cake's sharding model,
default.rs:11-130) — total work fixed, so "scaling": "strong".

Synthetic data: seeded-uniform token ids (seed 299792458 = cake's default,
lib.rs:180); random-init weights of the named architecture (no network).
With `--full` the oracle (CPU restatement) is timed beside it as
cpu_baseline — baseline only, never the target.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SEED = 299792458

# algorithmic bytes: streamed once per decode step
HBM_PEAK_GBS = 8000.0       # MI355X spec peak (MI355X_MICROARCH.md)
MFMA_PEAK_BF16_TF = 2500.0  # dense bf16 MFMA peak (never the 2:1-sparse 5PF)

# Per-launch HBM traffic of the dominant decode kernel, measured with
# rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE (separate passes) and the gfx950
# FETCH_SIZE x2 wide-coalesced-read correction (MI355X_MICROARCH.md §HBM).
# Source: profiles/r01_pmc_fetch_size.csv / r01_pmc_write_size.csv (8B),
# profiles/r02_pmc_*.csv (later rounds).  Keys are (model, kernel); a
# missing entry reports traffic=null (honest, not a guess).
PMC_TRAFFIC_BYTES = {
    ("llama3-8b", "gemv_gateup"): (114806.5 * 2 + 112.0) * 1024,
}


def model_dtype(cfg_json):
    """Compute dtype label from the model config (weight storage dtype;
    accumulation is f32 everywhere)."""
    qc = cfg_json.get("quantization_config") or {}
    return "fp8" if qc.get("quant_method") == "fp8" else "bf16"


def flops_per_token(cfg_json, with_head=True):
    """Algorithmic prefill/decode flops per token ~= 2 * weight elements on
    the matmul path (qkv + o + gate/up/down per layer, + lm_head)."""
    H, I = cfg_json["hidden_size"], cfg_json["intermediate_size"]
    V, L = cfg_json["vocab_size"], cfg_json["num_hidden_layers"]
    nh = cfg_json["num_attention_heads"]
    nkv = cfg_json["num_key_value_heads"]
    hd = cfg_json.get("head_dim") or H // nh
    per_layer = (nh + 2 * nkv) * hd * H + nh * hd * H + 3 * I * H
    total = L * per_layer + (V * H if with_head else 0)
    return 2.0 * total


def log(rank, *a):
    if rank == 0:
        print(*a, file=sys.stderr, flush=True)


def cpu_baseline(cfg_json, sample_layers=8, max_secs=45.0, prompt_len=128):
    """Oracle (numpy restatement, kind='port') decode rate on this host.

    Sample: greedy decode steps of the same architecture with a
    `prompt_len`-token context (the bench protocol's prompt length), weights
    stored f16 (converted f32 per op like the oracle's astype), with
    `sample_layers` distinct random layers reused cyclically to bound RAM
    (cache-neutral: one block is far larger than any L3).
    Rate is scaled to a full-model token.
    """
    from oracle import Config, LayerWeights, ModelWeights, OracleModel
    cfg = Config.from_json(cfg_json)
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    hd, nh, nkv = cfg.hd, cfg.num_attention_heads, cfg.num_key_value_heads
    rng = np.random.default_rng(SEED)

    def t(*shape):
        return (rng.standard_normal(shape, dtype=np.float32) * 0.02
                ).astype(np.float16)

    nlay = min(sample_layers, cfg.num_hidden_layers)
    layers = [LayerWeights(
        input_layernorm=np.ones(H, np.float16),
        post_attention_layernorm=np.ones(H, np.float16),
        q_proj=t(nh * hd, H), k_proj=t(nkv * hd, H), v_proj=t(nkv * hd, H),
        o_proj=t(H, nh * hd), gate_proj=t(I, H), up_proj=t(I, H),
        down_proj=t(H, I),
        q_norm=np.ones(hd, np.float16) if cfg.use_qk_norm else None,
        k_norm=np.ones(hd, np.float16) if cfg.use_qk_norm else None,
    ) for _ in range(nlay)]
    embed = t(V, H)
    w = ModelWeights(embed_tokens=embed, norm=np.ones(H, np.float16),
                     lm_head=embed if cfg.tie_word_embeddings else t(V, H),
                     layers=[layers[i % nlay]
                             for i in range(cfg.num_hidden_layers)])
    # distinct KV per layer index is handled by OracleModel's kv list
    model = OracleModel(cfg, w)
    prompt = list(rng.integers(0, V, size=prompt_len))
    model.generate_greedy(prompt, 1)  # prefill of the full prompt context
    # timed steps
    steps = 0
    t0 = time.perf_counter()
    while True:
        logits = model.forward(np.array([[steps % V]], dtype=np.int64),
                               prompt_len + 1 + steps)
        steps = steps + 1 if logits is not None else steps
        del logits
        el = time.perf_counter() - t0
        if el > max_secs or steps >= 4:
            break
    try:
        import multiprocessing
        cores = multiprocessing.cpu_count()
    except Exception:
        cores = 1
    return {
        "value": steps / el, "unit": "tok/s", "cores": cores, "kind": "port",
        "sample": (f"{steps} greedy decode steps, {prompt_len}-token "
                   f"context, f16 weights, {nlay} distinct layers reused "
                   f"cyclically"),
    }


def build_roofline(model, st, note=None):
    """Decode HBM roofline of the dominant kernel from a kernel_stats()
    dict (eager stats mode, hipEvent-timed)."""
    dom = max(st.items(), key=lambda kv: kv[1]["ms"])
    name, d = dom
    gbs = d["bytes"] / (d["ms"] * 1e-3) / 1e9 if d["ms"] > 0 else 0
    traffic = PMC_TRAFFIC_BYTES.get((model, name))
    return {
        "bound": "hbm", "achieved": round(gbs, 1),
        "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(gbs / HBM_PEAK_GBS, 4),
        "traffic": round(traffic) if traffic else None,
        "kernel": name,
        "per_launch_ms": round(d["ms"] / d["launches"], 5),
        "note": note or (
            "eager stats mode (graph replay disabled while timing): "
            "per-kernel sums exceed the graph-mode step time; per-kernel "
            "GB/s is unaffected"),
        "all_kernels": {k: {"ms": round(v["ms"], 3),
                            "launches": v["launches"],
                            "gbs": round(v["bytes"] / (v["ms"] * 1e-3)
                                         / 1e9, 1) if v["ms"] > 0
                            else 0}
                        for k, v in st.items()},
    }


def build_prefill_roofline(cfg_json, prefill_tok_s):
    """Prefill is MFMA-bound: achieved TF = tok/s x
    algorithmic flops/token; fraction vs the dense bf16 peak.  fp8 prefill
    currently dequantizes to bf16 scratch, so the bf16 peak is the bound
    either way."""
    if not prefill_tok_s:
        return None
    f = flops_per_token(cfg_json)
    tf = prefill_tok_s * f / 1e12
    return {"bound": "mfma", "achieved": round(tf, 1),
            "peak": MFMA_PEAK_BF16_TF, "unit": "TFLOP/s",
            "frac": round(tf / MFMA_PEAK_BF16_TF, 4),
            "flops_per_token": f}


def bench_one_model(model, steps, warmup, prompt_len, prefill_len, max_seq,
                    stats_steps, use_graph=True):
    """Single-GPU compact bench of one model (the matrix-mode unit):
    returns a dict with decode/prefill rates and both rooflines."""
    import cake_amd
    from cake_amd.configs import MODELS
    cfg_json = MODELS[model]
    flags = cake_amd.HAS_EMBED | cake_amd.HAS_HEAD
    if use_graph:
        flags |= cake_amd.USE_GRAPH
    eng = cake_amd.Engine(json.dumps(cfg_json), flags=flags, max_seq=max_seq,
                          max_batch_tokens=2048, device=0)
    try:
        eng.init_random(seed=SEED, scale=0.02)
        rng = np.random.default_rng(SEED)
        prompt = rng.integers(0, cfg_json["vocab_size"],
                              size=prompt_len).astype(np.uint32)
        eng.prefill(prompt)
        if warmup > 0:
            eng.decode(warmup)
        eng.sync()
        t0 = time.perf_counter()
        eng.decode(steps)
        eng.sync()
        elapsed = time.perf_counter() - t0
        roofline = None
        if stats_steps > 0:
            eng.set_stats(True)
            eng.decode(stats_steps)
            eng.sync()
            eng.set_stats(False)
            roofline = build_roofline(model, eng.kernel_stats()["kernels"])
            eng.stats_reset()
        prefill_tok_s = None
        if prefill_len > 0 and prefill_len <= max_seq:
            eng.reset()
            pf = rng.integers(0, cfg_json["vocab_size"],
                              size=prefill_len).astype(np.uint32)
            # two untimed warm passes: the first builds the per-shape GEMM
            # plans, the second captures the prefill hipGraph — the timed
            # pass below replays it (steady-state serving behavior)
            eng.prefill(pf)
            eng.sync()
            eng.reset()
            eng.prefill(pf)
            eng.sync()
            eng.reset()
            t0 = time.perf_counter()
            eng.prefill(pf)
            eng.sync()
            prefill_tok_s = prefill_len / (time.perf_counter() - t0)
        dtype = model_dtype(cfg_json)
        return {
            "value": round(steps / elapsed, 2),
            "ms_per_step": round(elapsed / steps * 1000, 4),
            "dtype": dtype,
            "workload": (f"{model}-decode" if model.endswith(dtype)
                         else f"{model}-{dtype}-decode"),
            "prefill_tok_s": round(prefill_tok_s, 1) if prefill_tok_s
            else None,
            "prefill_len": prefill_len,
            "prefill_roofline": build_prefill_roofline(cfg_json,
                                                       prefill_tok_s),
            "roofline": roofline,
        }
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline decode "
                         "rate: roofline stats (--stats-steps), prefill "
                         "rate (--prefill-len), CPU baseline, --matrix")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the token ids the "
                         "timed decode call returned to DIR/tokens.npy "
                         "(float64, one per step)")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--prefill-len", type=int, default=2048,
                    help="with --full: tokens for the prefill-rate "
                         "measurement (0=skip)")
    ap.add_argument("--max-seq", type=int, default=4096)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baseline leg")
    ap.add_argument("--stats-steps", type=int, default=8,
                    help="with --full: eager decode steps timed per kernel "
                         "for the roofline (0=skip)")
    ap.add_argument("--matrix", default="llama3-70b,qwen3-32b-fp8,qwen3-0.6b",
                    help="with --full: comma-separated extra BASELINE "
                         "configs benched "
                         "compactly at N=1 into the 'matrix' key of the one "
                         "JSON line ('' = none)")
    ap.add_argument("--matrix-steps", type=int, default=24)
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    n_gpus = max(world, args.gpus)
    if world > 1 and args.gpus != world:
        args.gpus = world

    import cake_amd
    from cake_amd.configs import MODELS, weight_bytes_bf16
    cfg_json = MODELS[args.model]
    L = cfg_json["num_hidden_layers"]

    dist = None
    if world > 1:
        import torch
        import torch.distributed as tdist
        dist = tdist
        dist.init_process_group("gloo")

    # contiguous pipeline ranges via the cake topology boundary
    # (topology.rs range expressions; equal split like default.rs would give
    # equal-TFLOPS workers)
    bounds = [round(L * r / world) for r in range(world + 1)]
    topo_yaml = "".join(
        f"rank{r}:\n  host: 127.0.0.1:{10128 + r}\n  layers:\n"
        f"    - model.layers.{bounds[r]}-{bounds[r + 1] - 1}\n"
        for r in range(world))
    flags = 0
    if rank == 0:
        flags |= cake_amd.HAS_EMBED | cake_amd.HAS_HEAD
    if not args.no_graph:
        flags |= cake_amd.USE_GRAPH

    log(rank, f"[bench] creating engine model={args.model} world={world} "
        f"rank={rank} layers={bounds[rank]}..{bounds[rank + 1]}")
    eng = cake_amd.Engine.from_topology(
        json.dumps(cfg_json), topo_yaml, f"rank{rank}", flags=flags,
        max_seq=args.max_seq, max_batch_tokens=2048, device=local_rank)
    t0 = time.perf_counter()
    eng.init_random(seed=SEED, scale=0.02)
    log(rank, f"[bench] random-init weights "
        f"({weight_bytes_bf16(cfg_json, bounds[rank], bounds[rank + 1], rank == 0, rank == 0) / 1e9:.2f} GB shard) "
        f"in {time.perf_counter() - t0:.2f}s")

    if world > 1:
        import torch
        if rank == 0:
            cid = cake_amd.comm_id()
            tens = torch.tensor(bytearray(cid), dtype=torch.uint8)
        else:
            tens = torch.zeros(cake_amd.COMM_ID_BYTES, dtype=torch.uint8)
        dist.broadcast(tens, src=0)
        eng.comm_init(rank, world, bytes(tens.numpy().tobytes()))

    rng = np.random.default_rng(SEED)
    prompt = rng.integers(0, cfg_json["vocab_size"],
                          size=args.prompt_len).astype(np.uint32)

    def barrier_sync():
        eng.sync()
        if dist:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize(local_rank)
            dist.barrier()

    # ---- prefill the prompt + warmup ------------------------------------
    if rank == 0:
        eng.prefill(prompt)
    else:
        eng.prefill_participate(len(prompt))
    if args.warmup > 0:
        if rank == 0:
            eng.decode(args.warmup)
        else:
            eng.decode_participate(args.warmup)
    barrier_sync()

    # ---- timed decode region (the headline metric) ----------------------
    t0 = time.perf_counter()
    if rank == 0:
        toks = eng.decode(args.steps)
    else:
        eng.decode_participate(args.steps)
    barrier_sync()
    elapsed = time.perf_counter() - t0
    if dist:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    decode_tok_s = args.steps / elapsed
    log(rank, f"[bench] decode: {args.steps} steps in {elapsed:.3f}s = "
        f"{decode_tok_s:.1f} tok/s")

    # ---- what the timed call returned, for build-to-build comparison ------
    if rank == 0 and args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "tokens.npy"),
                np.asarray(toks, dtype=np.float64))
        log(rank, f"[bench] wrote {len(toks)} token ids to "
            f"{os.path.join(args.dump_outputs, 'tokens.npy')}")

    # ---- everything below is a --full leg --------------------------------
    # ---- roofline stats segment (eager, hipEvent-timed) ------------------
    roofline = None
    if args.full and args.stats_steps > 0:
        eng.set_stats(True)
        if rank == 0:
            eng.decode(args.stats_steps)
        else:
            eng.decode_participate(args.stats_steps)
        barrier_sync()
        eng.set_stats(False)
        if rank == 0:
            roofline = build_roofline(args.model,
                                      eng.kernel_stats()["kernels"])
        eng.stats_reset()

    # ---- prefill rate ----------------------------------------------------
    prefill_tok_s = None
    if args.full and 0 < args.prefill_len <= args.max_seq:
        pf = rng.integers(0, cfg_json["vocab_size"],
                          size=args.prefill_len).astype(np.uint32)
        # two untimed warm passes: the first builds the per-shape GEMM
        # plans, the second captures the prefill hipGraph; the timed pass
        # below replays it (steady-state serving behavior, same as the
        # matrix models' bench_one_model)
        for _ in range(2):
            eng.reset()
            if rank == 0:
                eng.prefill(pf)
            else:
                eng.prefill_participate(len(pf))
            barrier_sync()
        eng.reset()
        barrier_sync()
        t0 = time.perf_counter()
        if rank == 0:
            eng.prefill(pf)
        else:
            eng.prefill_participate(len(pf))
        barrier_sync()
        el = time.perf_counter() - t0
        if dist:
            import torch
            t = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        prefill_tok_s = args.prefill_len / el
        log(rank, f"[bench] prefill: {args.prefill_len} tokens in {el:.3f}s "
            f"= {prefill_tok_s:.0f} tok/s")

    # ---- CPU baseline (rank 0, N=1 only) ---------------------------------
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        log(rank, "[bench] timing CPU baseline (oracle, bounded sample) ...")
        cpu = cpu_baseline(cfg_json, prompt_len=args.prompt_len)
        log(rank, f"[bench] cpu_baseline: {cpu['value']:.3f} tok/s on "
            f"{cpu['cores']} cores")

    # ---- matrix mode: the other BASELINE configs, compactly (N=1 only) ---
    matrix = None
    if args.full and rank == 0 and world == 1 and args.matrix:
        matrix = {}
        for m in [s for s in args.matrix.split(",") if s]:
            if m == args.model:
                continue
            log(rank, f"[bench] matrix: {m} ...")
            try:
                matrix[m] = bench_one_model(
                    m, steps=args.matrix_steps, warmup=6,
                    prompt_len=args.prompt_len,
                    prefill_len=min(512, args.max_seq),
                    max_seq=args.max_seq, stats_steps=4,
                    use_graph=not args.no_graph)
                log(rank, f"[bench] matrix {m}: "
                    f"{matrix[m]['value']} tok/s decode, "
                    f"{matrix[m]['prefill_tok_s']} tok/s prefill")
            except Exception as e:
                matrix[m] = {"error": str(e)}
                log(rank, f"[bench] matrix {m} FAILED: {e}")

    if rank == 0:
        dtype = model_dtype(cfg_json)
        out = {
            "metric": "decode tok/s",
            "value": round(decode_tok_s, 2),
            "unit": "tok/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": dtype,
            "data": "synthetic",
            "config": {
                "workload": (f"{args.model}-decode" if args.model.endswith(dtype)
                         else f"{args.model}-{dtype}-decode"),
                "model": args.model,
                "prompt_len": args.prompt_len,
                "gen_tokens": args.steps,
                "parallelism": f"pp{n_gpus}",
            },
            "prefill_tok_s": round(prefill_tok_s, 1) if prefill_tok_s else None,
            "prefill_len": args.prefill_len if args.full else None,
            "prefill_roofline": build_prefill_roofline(cfg_json,
                                                       prefill_tok_s),
            "roofline": roofline,
            "cpu_baseline": cpu,
            "matrix": matrix,
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
