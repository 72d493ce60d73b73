"""OpenAI-compatible serving front-end over the MI355X engine.

Mirrors cake's API surface (cake-core/src/cake/sharding/api/mod.rs:66-110):
  POST /v1/chat/completions   (streaming SSE + non-streaming, api/text.rs)
  POST /v1/completions
  GET  /v1/models
  GET  /api/v1/topology       (api/mod.rs:104-107)

Generation is the same hot loop the bench measures (Master::generate_text,
master.rs:109-171): greedy ArgMax when temperature <= 0, on-GPU
Gumbel-argmax sampling for plain temperature (cake's own
temperature-sampling trick, text_model.rs:102-118).  top_k / top_p /
repeat_penalty / repeat_last_n requests stay on that loop too: the engine's
set_sampling_ex runs the penalty (text_model.rs:433-452), the top-k and
top-p selection and the seeded draw on the GPU inside the decode graph.
Only an engine without set_sampling_ex falls back to the host-sampling loop
over per-token logits (one append-prefill and one logits copy per token).

Tokenization: pass a `tokenizers.Tokenizer` (tokenizer.json) for text
prompts; without one, requests supply `prompt_token_ids` directly (the
engine-level contract).  Chat messages are flattened with a minimal
"role: content" template when no chat template is available.

Run:  python -m cake_amd.serve --model llama3-8b --port 8000
(random-init weights unless --safetensors is given — there is no network
for checkpoints in this environment).
"""
import argparse
import json
import time
import uuid
from typing import Optional

import numpy as np


def build_prompt(messages):
    # minimal template; serving real chats needs the model's own chat
    # template (out of round-1 scope)
    parts = [f"{m.get('role', 'user')}: {m.get('content', '')}"
             for m in messages]
    parts.append("assistant:")
    return "\n".join(parts)


def sample_from_logits(logits, temperature, top_k, top_p, rng):
    """Restates candle's Sampling::{TopK,TopP,TopKThenTopP,All} as cake
    configures it (text_model.rs:102-118): softmax at `temperature`, keep
    the top-k, then the minimal nucleus reaching top_p (always >= 1
    token), renormalize, multinomial draw."""
    x = np.asarray(logits, dtype=np.float64) / max(1e-6, temperature)
    x -= x.max()
    p = np.exp(x)
    p /= p.sum()
    order = np.argsort(-p)
    if top_k:
        order = order[:int(top_k)]
    kept = p[order]
    if top_p and top_p < 1.0:
        c = np.cumsum(kept) / kept.sum()
        cut = int(np.searchsorted(c, top_p)) + 1
        order = order[:cut]
        kept = kept[:cut]
    kept = kept / kept.sum()
    return int(rng.choice(order, p=kept))


def apply_repeat_penalty(logits, penalty, ids):
    """cake's sign-aware repeat penalty (text_model.rs:51-99): each unique
    id is scaled once, l / penalty if l >= 0 else l * penalty."""
    out = np.array(logits, dtype=np.float32)
    idx = np.unique(np.asarray(ids, dtype=np.int64))
    v = out[idx]
    out[idx] = np.where(v >= 0, v * np.float32(1.0 / penalty),
                        v * np.float32(penalty))
    return out


class GenSession:
    """Thin generation driver over an Engine-compatible object.

    The engine only needs: reset(), prefill(ids)->int, decode(n)->list[int].
    """

    def __init__(self, engine, eos_ids=(), chunk=8):
        self.engine = engine
        self.eos_ids = set(int(e) for e in eos_ids)
        self.chunk = chunk

    def generate(self, prompt_ids, max_tokens):
        """Yield token ids, stopping at EOS or max_tokens (the per-token
        stream Master::generate_text hands its callback, master.rs:125-168)."""
        self.engine.reset()
        first = int(self.engine.prefill(np.asarray(prompt_ids,
                                                   dtype=np.uint32)))
        produced = 0
        tok = first
        while True:
            yield tok
            produced += 1
            if produced >= max_tokens or tok in self.eos_ids:
                return
            n = min(self.chunk, max_tokens - produced)
            toks = self.engine.decode(n)
            for i, t in enumerate(toks):
                t = int(t)
                if i == len(toks) - 1:
                    tok = t
                    break
                yield t
                produced += 1
                if produced >= max_tokens or t in self.eos_ids:
                    return

    def generate_sampled(self, prompt_ids, max_tokens, temperature, top_k,
                         top_p, seed, repeat_penalty=1.0, repeat_last_n=0):
        """Host-sampling fallback for engines without set_sampling_ex:
        per-token logits from append-prefill steps, sampled like cake's
        host-side LogitsProcessor (far slower than the graph-replayed
        decode loop).  The repeat penalty covers generated tokens only."""
        self.engine.reset()
        rng = np.random.default_rng(seed)
        _, logits = self.engine.prefill(
            np.asarray(prompt_ids, dtype=np.uint32), want_logits=True)
        produced = 0
        history = []
        while True:
            if repeat_penalty != 1.0 and repeat_last_n > 0 and history:
                logits = apply_repeat_penalty(logits, repeat_penalty,
                                              history[-repeat_last_n:])
            if temperature > 0:
                tok = sample_from_logits(logits, temperature, top_k, top_p,
                                         rng)
            else:
                tok = int(np.argmax(logits))
            history.append(tok)
            yield tok
            produced += 1
            if produced >= max_tokens or tok in self.eos_ids:
                return
            _, logits = self.engine.prefill(
                np.asarray([tok], dtype=np.uint32), want_logits=True)


def create_app(engine, model_name="cake-amd", tokenizer=None, eos_ids=(),
               topology=None):
    import threading

    from fastapi import FastAPI, Request
    from fastapi.responses import JSONResponse, StreamingResponse
    from starlette.concurrency import run_in_threadpool

    app = FastAPI(title="cake_amd")
    sess = GenSession(engine, eos_ids=eos_ids)
    # ONE engine = ONE KV sequence: the reference serializes generations by
    # wrapping Master in Arc<RwLock> (api/text.rs:102).  The lock is held for
    # the FULL generation including SSE streaming; both the streaming
    # generator and the non-streaming list() run in starlette's threadpool,
    # so a blocking acquire here never stalls the event loop.
    engine_lock = threading.Lock()

    def encode(text):
        if tokenizer is None:
            raise ValueError(
                "no tokenizer loaded — pass prompt_token_ids instead")
        return tokenizer.encode(text).ids

    def decode_tok(tok):
        if tokenizer is None:
            return f"<{tok}>"
        return tokenizer.decode([tok])

    @app.get("/v1/models")
    def models():  # api/mod.rs route
        return {"object": "list",
                "data": [{"id": model_name, "object": "model",
                          "owned_by": "cake_amd"}]}

    @app.get("/api/v1/topology")
    def topo():  # api/mod.rs:104-107
        return topology or {}

    async def run_request(body, kind):
        max_tokens = int(body.get("max_tokens", 128))
        stream = bool(body.get("stream", False))
        temperature = float(body.get("temperature", 0.0))
        top_k = body.get("top_k")
        top_p = body.get("top_p")
        seed = int(body.get("seed", 299792458))
        repeat_penalty = float(body.get("repeat_penalty", 1.0))
        # the engine's history ring holds 1024 ids
        repeat_last_n = max(0, min(1024, int(body.get("repeat_last_n", 128))))
        wants_ex = bool(
            (temperature > 0 and (top_k or (top_p and top_p < 1.0))) or
            (repeat_penalty != 1.0 and repeat_last_n > 0))
        # on the device when the engine can; else the host loop
        on_device = wants_ex and hasattr(engine, "set_sampling_ex")
        use_host_sampling = wants_ex and not on_device
        if "prompt_token_ids" in body:
            ids = [int(t) for t in body["prompt_token_ids"]]
        elif kind == "chat":
            ids = encode(build_prompt(body.get("messages", [])))
        else:
            ids = encode(body.get("prompt", ""))
        rid = f"chatcmpl-{uuid.uuid4().hex[:12]}"
        created = int(time.time())

        def gen_stream():
            """Engine-touching generator; holds the engine lock from before
            the first engine call until exhaustion (or client disconnect —
            GeneratorExit releases it through the `with`)."""
            with engine_lock:
                if on_device:
                    engine.set_sampling_ex(
                        temperature, top_k=int(top_k or 0),
                        top_p=float(top_p) if top_p else 1.0,
                        repeat_penalty=repeat_penalty,
                        repeat_last_n=repeat_last_n, seed=seed)
                elif (not use_host_sampling and
                      hasattr(engine, "set_sampling")):
                    engine.set_sampling(temperature, seed)
                if use_host_sampling:
                    gen = sess.generate_sampled(
                        ids, max_tokens, temperature, top_k, top_p, seed,
                        repeat_penalty=repeat_penalty,
                        repeat_last_n=repeat_last_n)
                else:
                    gen = sess.generate(ids, max_tokens)
                for tok in gen:
                    yield tok

        if stream:
            def sse():
                for tok in gen_stream():
                    delta = ({"content": decode_tok(tok)} if kind == "chat"
                             else None)
                    chunk = {
                        "id": rid, "object": "chat.completion.chunk",
                        "created": created, "model": model_name,
                        "choices": [{
                            "index": 0,
                            "delta": delta if kind == "chat" else None,
                            "text": (None if kind == "chat"
                                     else decode_tok(tok)),
                            "token_id": int(tok),
                            "finish_reason": None,
                        }],
                    }
                    yield f"data: {json.dumps(chunk)}\n\n"
                yield "data: [DONE]\n\n"
            return StreamingResponse(sse(), media_type="text/event-stream")

        # blocking generation off the event loop (api/text.rs's non-stream
        # path holds its lock inside a spawned task, not the acceptor)
        toks = await run_in_threadpool(lambda: list(gen_stream()))
        text = ("".join(decode_tok(t) for t in toks) if tokenizer
                else None)
        finish = "stop" if (toks and toks[-1] in sess.eos_ids) else "length"
        if kind == "chat":
            choice = {"index": 0, "finish_reason": finish,
                      "message": {"role": "assistant", "content": text},
                      "token_ids": [int(t) for t in toks]}
        else:
            choice = {"index": 0, "finish_reason": finish, "text": text,
                      "token_ids": [int(t) for t in toks]}
        return JSONResponse({
            "id": rid, "object": "chat.completion", "created": created,
            "model": model_name, "choices": [choice],
            "usage": {"prompt_tokens": len(ids),
                      "completion_tokens": len(toks),
                      "total_tokens": len(ids) + len(toks)},
        })

    @app.post("/v1/chat/completions")
    async def chat(request: Request):
        return await run_request(await request.json(), "chat")

    @app.post("/v1/completions")
    async def completions(request: Request):
        return await run_request(await request.json(), "completions")

    return app


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b",
                    help="a name from configs.MODELS, QUANT_MODELS, "
                    "QWEN2_MODELS, PHI_MODELS, FALCON3_MODELS or "
                    "GEMMA3_MODELS (e.g. phi-4-mini, falcon3-7b, "
                    "gemma-3-4b)")
    ap.add_argument("--safetensors", default=None)
    ap.add_argument("--tokenizer", default=None,
                    help="path to a tokenizer.json")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--max-seq", type=int, default=4096)
    args = ap.parse_args()

    import cake_amd
    from cake_amd.configs import find_model
    cfg = find_model(args.model)
    eng = cake_amd.Engine(json.dumps(cfg), max_seq=args.max_seq,
                          max_batch_tokens=2048)
    if args.safetensors:
        eng.load_safetensors(args.safetensors)
    else:
        eng.init_random()
    tok = None
    if args.tokenizer:
        from tokenizers import Tokenizer
        tok = Tokenizer.from_file(args.tokenizer)
    eos = cfg.get("eos_token_id")
    eos_ids = ([eos] if isinstance(eos, int) else (eos or []))
    app = create_app(eng, model_name=args.model, tokenizer=tok,
                     eos_ids=eos_ids)

    import uvicorn
    uvicorn.run(app, host=args.host, port=args.port)


if __name__ == "__main__":
    main()
