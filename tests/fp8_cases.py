"""The fp8 engine cases: configs, the synthetic checkpoint builder, the
reference and its mutants, the prompt seeds and the hidden-state protocol.
Shared by tests/test_fp8_engine_gpu.py (runs the engine on them) and
tests/test_fp8_ref.py (shows on the CPU that the same inputs have teeth), so it
imports nothing that needs the native library.

The reference is oracle.OracleModel (tests/qwen2_ref.Qwen2Oracle for the bias
family) on the dequantized weights rounded to bf16, as the prefill path stores
them: the pattern of test_gpu_parity.quantized_oracle.  It is rebuilt from the
very tensors that are written to the checkpoint, so a mutant is a change to
how those tensors are read and to nothing else.

Every H, I, Sq and Skv is a multiple of 128; these are the smallest shapes that
reach each route:
  llama_hd64      per-head decode attention; non-square scale grids (gate 3x2,
                  down 2x3); k and v parts at block-rows 2 and 3 of the qkv grid
  qwen3_hd128     QK-norm, tied embeddings
  qwen3_hd64_swa  QK-norm, window 16 on layer 1 only (max_window_layers 1)
  qwen2_hd64      q/k/v bias
  mistral_hd128   window 16 on every layer, grouped decode attention (G = 4)
  wide_mlp        down K = 16640 > 16384: the streaming GEMV, residual aliased
  wide_hidden     qkv / gate-up K = 4224: KB 2 with a 128-wide tail
"""
import functools

import numpy as np

from oracle import (Config, LayerWeights, ModelWeights, OracleModel,
                    f8e4m3_to_f32)
from tests import qwen2_ref as qr
from tests.helpers import quantize_bf16

GATE = 3e-2          # the project's fp8 logits gate (test_fp8_engine_parity)
TEETH = 4 * GATE     # what a mutant has to move an observable by
PROMPT_LEN = 40      # > the window of 16: it clips in prefill and in decode
GEN = 8              # greedy ids compared with the reference
MAX_SEQ = 128
MAX_BATCH_TOKENS = 64
WINDOW = 16
BLOCK = 128
HID_ROWS = 12        # forward_hidden: 12 rows at position 0 ...
HID_STEPS = 8        # ... then single rows at 12..19, across the window


def _cfg(model_type, H, I, nh, nkv, hd, L=2, V=512, **extra):
    j = dict(model_type=model_type, hidden_size=H, intermediate_size=I,
             vocab_size=V, num_hidden_layers=L, num_attention_heads=nh,
             num_key_value_heads=nkv, head_dim=hd, rms_norm_eps=1e-6,
             rope_theta=1000000.0, max_position_embeddings=512,
             tie_word_embeddings=False,
             quantization_config=dict(quant_method="fp8",
                                      weight_block_size=[BLOCK, BLOCK]))
    j.update(extra)
    return j


CONFIGS = {
    "llama_hd64": _cfg("llama", 256, 384, 4, 2, 64),
    "qwen3_hd128": _cfg("qwen3", 256, 384, 2, 1, 128,
                        tie_word_embeddings=True),
    "qwen3_hd64_swa": _cfg("qwen3", 256, 384, 4, 2, 64, sliding_window=WINDOW,
                           use_sliding_window=True, max_window_layers=1),
    "qwen2_hd64": _cfg("qwen2", 256, 384, 4, 2, 64),
    "mistral_hd128": _cfg("mistral", 256, 384, 4, 1, 128,
                          sliding_window=WINDOW),
    "wide_mlp": _cfg("llama", 256, 16640, 2, 1, 128, L=1),
    "wide_hidden": _cfg("llama", 4224, 128, 1, 1, 128, L=1, V=256),
}
NAMES = tuple(CONFIGS)
MODEL_SEED = {n: 101 + i for i, n in enumerate(NAMES)}

# The spread of the block scales (build_model's octaves).  With the helper's
# 3e-4 .. 5e-4 two blocks differ by 5/3 at most, and on three configs a scale
# mutant moved an observable by less than TEETH: kv_scale_swap the logits of
# qwen3_hd128 by 0.101 and of wide_mlp by 0.087, gateup_scale_swap the hidden
# state of mistral_hd128 by 0.102.  Those three take one more octave, the least
# that brings every mutant above TEETH.  The others keep the helper's spread:
# larger weights sharpen the softmax, and with it the error that bf16 storage
# of the activations alone makes against an f32 reference grows (qwen2_hd64
# with its large biases: 0.014 of the hidden state at one octave, 0.052 at two,
# above the gate; test_fp8_ref.py holds that emulation).
SCALE_OCTAVES = {"qwen3_hd128": 2, "mistral_hd128": 2, "wide_mlp": 2}

# The first prompt seed of 0, 1, 2, ... at which the reference's two largest
# logits stay at least 2 * GATE * max|logits| apart at each of the GEN greedy
# steps (find_prompt_seed; test_fp8_ref.py asserts the condition, it does not
# search).  While the engine's logits are inside GATE no argmax can flip, so
# the greedy tests compare ids exactly.
PROMPT_SEED = {
    "llama_hd64": 10,
    "qwen3_hd128": 94,
    "qwen3_hd64_swa": 78,
    "qwen2_hd64": 80,
    "mistral_hd128": 31,
    "wide_mlp": 25,
    "wide_hidden": 12,
}

PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj",
        "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-9, np.max(np.abs(b))))


def proj_shapes(cfg: Config) -> dict:
    H, I = cfg.hidden_size, cfg.intermediate_size
    sq = cfg.num_attention_heads * cfg.hd
    skv = cfg.num_key_value_heads * cfg.hd
    return dict(zip(PROJ, ((sq, H), (skv, H), (skv, H), (H, sq), (I, H),
                           (I, H), (H, I))))


# ---- the builder ---------------------------------------------------------------
def build_model(cfg_json: dict, seed: int, octaves: int = 1,
                exact_scales: bool = False):
    """A synthetic fp8 checkpoint of any supported family: returns (tensors,
    reference).  tests/helpers.random_fp8_model generalised: e4m3fn bytes
    without NaN codes and one weight_scale_inv per 128 x 128 block, plus
    q_norm / k_norm weights far from 1 for qwen3 and the q/k/v biases of
    qwen2_ref.random_biases for qwen2; tie_word_embeddings is honoured.

    Scales are (3e-4 .. 5e-4) * 2^u, u in 0 .. octaves-1 drawn per block:
    octaves = 1 is the helper's spread (SCALE_OCTAVES says which configs take
    more and why).  exact_scales rounds them to bf16, which in this range is
    f16-exact too."""
    cfg = Config.from_json(cfg_json)
    rng = np.random.default_rng(seed)
    H, V, hd = cfg.hidden_size, cfg.vocab_size, cfg.hd

    def f32(*shape):
        return (rng.standard_normal(shape) * 0.02).astype(np.float32)

    tensors = {}
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        for name, (n, k) in proj_shapes(cfg).items():
            b = rng.integers(0, 256, size=(n, k)).astype(np.uint8)
            b[(b & 0x7F) == 0x7F] ^= 0x08            # no NaN encodings
            grid = (n // BLOCK, k // BLOCK)
            sc = ((3e-4 + 2e-4 * rng.random(grid)) *
                  2.0 ** rng.integers(0, octaves, size=grid)
                  ).astype(np.float32)
            tensors[p + name + ".weight"] = b
            tensors[p + name + ".weight_scale_inv"] = (
                quantize_bf16(sc) if exact_scales else sc)
        tensors[p + "input_layernorm.weight"] = 1.0 + f32(H)
        tensors[p + "post_attention_layernorm.weight"] = 1.0 + f32(H)
        if cfg.use_qk_norm:
            for nm in ("q_norm", "k_norm"):
                tensors[p + f"self_attn.{nm}.weight"] = quantize_bf16(
                    (1.0 + 0.5 * rng.standard_normal(hd)).astype(np.float32))
    tensors["model.embed_tokens.weight"] = f32(V, H)
    tensors["model.norm.weight"] = 1.0 + f32(H)
    if not cfg.tie_word_embeddings:
        tensors["lm_head.weight"] = f32(V, H)
    if cfg_json["model_type"] == "qwen2":
        tensors.update(qr.bias_tensors(qr.random_biases(cfg, seed + 1), cfg))
    return tensors, reference(cfg_json, tensors)


# ---- the reference and its mutants ---------------------------------------------
SCALE_MUTANTS = ("kv_scale_swap", "gateup_scale_swap", "block_row0",
                 "scale_stride")


def mutants_of(name: str) -> tuple:
    """The mutants that apply to a config.  scale_stride needs a grid with
    more than one row and one column whose sides differ: on wide_hidden every
    grid is a single row or a single column, where any row stride reads the
    same scale, so the mutant is the identity there and is left out."""
    j = CONFIGS[name]
    grids = [(n // BLOCK, k // BLOCK)
             for n, k in proj_shapes(Config.from_json(j)).values()]
    out = [m for m in SCALE_MUTANTS if m != "scale_stride" or
           any(a != b and min(a, b) > 1 for a, b in grids)]
    if "qwen3" in j["model_type"]:
        out += ["no_q_norm", "no_k_norm", "no_qk_norm"]
    if j["model_type"] == "qwen2":
        out += ["no_q_bias", "no_k_bias", "no_v_bias"]
    if j.get("sliding_window"):
        out.append("no_window")
        if j.get("max_window_layers"):
            out.append("window_on_layer0")
    if j.get("tie_word_embeddings"):
        out.append("untied_head")
    return tuple(out)


def dequant(w8, sc):
    """utils/fp8.rs:42-64: w[i, j] = e4m3fn(w8[i, j]) * sc[i // 128, j // 128]."""
    table = f8e4m3_to_f32(np.arange(256, dtype=np.uint8))
    big = np.repeat(np.repeat(sc.astype(np.float32), BLOCK, axis=0), BLOCK,
                    axis=1)
    return (table[w8] * big).astype(np.float32)


def _scales(tensors, p, mutant):
    """The seven scale grids of layer prefix p as the (mutated) reader sees
    them."""
    s = {n: tensors[p + n + ".weight_scale_inv"] for n in PROJ}
    q, k, v = PROJ[:3]
    gate, up = PROJ[4], PROJ[5]
    if mutant == "kv_scale_swap":
        s[k], s[v] = s[v], s[k]
    elif mutant == "gateup_scale_swap":
        s[gate], s[up] = s[up], s[gate]
    elif mutant == "block_row0":
        # every part of a fused projection reads the fused grid from its
        # block-row 0 on (the part's row offset ignored): k and v get q's
        # first rows, up gets gate's
        s[k] = s[q][:s[k].shape[0]]
        s[v] = s[q][:s[v].shape[0]]
        s[up] = s[gate]
    elif mutant == "scale_stride":
        # the (N/128, K/128) grid walked with row stride N/128 instead of
        # K/128, wherever the two differ
        for n in PROJ:
            nb, kb = s[n].shape
            if nb != kb:
                s[n] = s[n].reshape(kb, nb).T
    return s


def reference(cfg_json: dict, tensors: dict, mutant: str = None):
    """The oracle on what `tensors` holds, weights rounded to bf16; with
    `mutant`, on what a reader with that one defect would make of them."""
    cfg = Config.from_json(cfg_json)
    if mutant == "no_window":
        cfg.sliding_window = cfg.layer_windows = None
    elif mutant == "window_on_layer0":
        cfg.layer_windows = (cfg.layer_windows[1], None)
    q = quantize_bf16
    layers = []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        sc = _scales(tensors, p, mutant)
        w = [q(dequant(tensors[p + n + ".weight"], sc[n])) for n in PROJ]
        qn = tensors.get(p + "self_attn.q_norm.weight")
        kn = tensors.get(p + "self_attn.k_norm.weight")
        if mutant in ("no_q_norm", "no_qk_norm"):
            qn = None
        if mutant in ("no_k_norm", "no_qk_norm"):
            kn = None
        layers.append(LayerWeights(
            q(tensors[p + "input_layernorm.weight"]),
            q(tensors[p + "post_attention_layernorm.weight"]), *w,
            q_norm=None if qn is None else q(qn),
            k_norm=None if kn is None else q(kn)))
    embed = q(tensors["model.embed_tokens.weight"])
    head = embed if cfg.tie_word_embeddings else q(tensors["lm_head.weight"])
    if mutant == "untied_head":
        head = q((np.random.default_rng(977).standard_normal(embed.shape)
                  * 0.02).astype(np.float32))
    w = ModelWeights(embed_tokens=embed, norm=q(tensors["model.norm.weight"]),
                     lm_head=head, layers=layers)
    if cfg_json["model_type"] != "qwen2":
        return OracleModel(cfg, w)
    biases = qr.fused_biases(tensors, cfg)       # f32 on the device too
    if mutant in ("no_q_bias", "no_k_bias", "no_v_bias"):
        biases = qr.drop_one(biases, cfg, mutant[3])
    return qr.Qwen2Oracle(cfg, w, biases)


# ---- the observables -------------------------------------------------------------
def observables_of(mutant: str) -> tuple:
    """What a mutant can move: the head is no part of forward_hidden, so
    untied_head shows in the logits alone."""
    return ("logits",) if mutant == "untied_head" else ("logits", "hidden")


def prompt_of(name: str, seed: int = None) -> np.ndarray:
    seed = PROMPT_SEED[name] if seed is None else seed
    return np.random.default_rng(seed).integers(
        0, CONFIGS[name]["vocab_size"], size=PROMPT_LEN).astype(np.uint32)


def prefill_logits(ref, prompt) -> np.ndarray:
    ref.reset()
    return ref.forward(np.asarray(prompt, dtype=np.int64)[None, :], 0)[0]


def greedy_gaps(ref, prompt, steps: int = GEN):
    """(ids, gaps): the reference's greedy ids and, per step, the gap of its
    two largest logits over max|logits|."""
    ref.reset()
    ids, gaps = [], []
    ctx, pos = [int(t) for t in prompt], 0
    for _ in range(steps):
        lg = ref.forward(np.array([ctx], dtype=np.int64), pos)[0]
        pos += len(ctx)
        top = np.sort(lg)
        gaps.append(float((top[-1] - top[-2]) / np.max(np.abs(lg))))
        ids.append(int(np.argmax(lg)))
        ctx = [ids[-1]]
    return ids, gaps


def find_prompt_seed(name: str, ref, steps: int = GEN, limit: int = 500):
    """How PROMPT_SEED was chosen."""
    for seed in range(limit):
        if min(greedy_gaps(ref, prompt_of(name, seed), steps)[1]) >= 2 * GATE:
            return seed
    return None


def hidden_inputs(name: str):
    """(x12, xs): 12 rows for position 0 and 8 single rows for positions
    12..19, bf16-exact so the engine's input conversion changes nothing."""
    H = CONFIGS[name]["hidden_size"]
    rng = np.random.default_rng(4242)
    x = quantize_bf16((rng.standard_normal((HID_ROWS + HID_STEPS, H)) * 0.05
                       ).astype(np.float32))
    return x[:HID_ROWS], x[HID_ROWS:]


def hidden_outputs(ref, name: str, lo: int = 0, hi: int = None):
    """The reference's side of the hidden-state protocol: [(12, H)] + 8 x
    [(1, H)] outputs of blocks [lo, hi)."""
    hi = ref.cfg.num_hidden_layers if hi is None else hi
    x12, xs = hidden_inputs(name)
    ref.reset()
    out = [ref.hidden_forward(x12[None], 0, lo, hi)[0]]
    for i in range(HID_STEPS):
        out.append(ref.hidden_forward(xs[i][None, None], HID_ROWS + i, lo,
                                      hi)[0])
    return out


@functools.lru_cache(maxsize=None)
def case(name: str):
    """Everything the tests of one config share, computed once: do not
    modify."""
    cfg_json = CONFIGS[name]
    tensors, ref = build_model(cfg_json, MODEL_SEED[name],
                               SCALE_OCTAVES.get(name, 1))
    prompt = prompt_of(name)
    ids, gaps = greedy_gaps(ref, prompt)
    return dict(cfg_json=cfg_json, tensors=tensors, ref=ref, prompt=prompt,
                logits=prefill_logits(ref, prompt), ids=ids, gaps=gaps,
                hidden=hidden_outputs(ref, name))
