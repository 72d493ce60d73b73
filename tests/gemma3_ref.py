"""The oracle for gemma3 (HF transformers' Gemma3ForCausalLM, text only):
oracle.OracleModel with the family's differences.

  * four norms per layer, every norm weight in the (1 + w) form: the two
    post norms act on the attention / MLP output ahead of the residual add;
  * QK-norm (also 1 + w), scores scaled by query_pre_attn_scalar^-0.5;
  * local (sliding-window) and global layers in any order, each kind with its
    own rope table; rope type "linear" divides the frequencies by its factor;
  * gelu_pytorch_tanh gate; embedding rows times sqrt(hidden); tied head.

`DEFECTS` are the ways an engine gets this family wrong;
tools/gen_golden_gemma3.py builds tests/golden/tiny_gemma3 so that each moves
the logits by at least four times the engine tests' 2e-2 gate, and
tests/test_gemma3_ref.py checks that on the committed file.

The fixture's npz holds the checkpoint's own tensors ("w." + the HF name, the
norm rows as stored: w, not 1 + w).  Test infrastructure only, like oracle/."""
import json
import math
import os

import numpy as np

from oracle import (Config, OracleModel, causal_mask, linear, rms_norm, rope,
                    silu_mul, softmax_lastdim)
from tests.phi3_ref import _bf16

DEFECTS = (
    "plain_w_norms",       # w instead of 1 + w in every norm
    "no_post_norms",       # the two post norms skipped
    "silu_gate",           # SiLU instead of GELU-tanh
    "no_embed_scale",      # embedding rows not scaled by sqrt(H)
    "global_theta_all",    # every layer on the global layers' rope
    "linear_ignored",      # the linear rope factor dropped
    "local_no_rope",       # local layers not rotated (the reference's way)
    "all_global",          # every layer full attention, global rope
    "all_local",           # every layer windowed, local rope
    "hd_scale",            # scores times head_dim^-0.5
)


def text_config(cfg_json: dict) -> dict:
    """The text model's fields with HF's Gemma3TextConfig defaults, from a
    gemma3_text config or a gemma3 one with a nested text_config."""
    j = cfg_json
    if j.get("model_type") == "gemma3":
        j = dict(j.get("text_config") or {})
    d = dict(vocab_size=262208, hidden_size=2304, intermediate_size=9216,
             num_hidden_layers=26, num_attention_heads=8,
             num_key_value_heads=4, head_dim=256, rms_norm_eps=1e-6,
             max_position_embeddings=131072, sliding_window=4096,
             query_pre_attn_scalar=256)
    d.update({k: v for k, v in j.items() if v is not None or k not in d})
    return d


def layer_kinds(cfg_json: dict) -> list:
    """True per local (sliding) layer: layer_types, else layer i is global
    iff (i + 1) % sliding_window_pattern == 0 (pattern 6 by default)."""
    t = text_config(cfg_json)
    if t.get("layer_types"):
        return [k == "sliding_attention" for k in t["layer_types"]]
    pat = t.get("sliding_window_pattern", 6)
    return [bool((i + 1) % pat) for i in range(t["num_hidden_layers"])]


def rope_params(cfg_json: dict, local: bool) -> tuple:
    """(theta, linear factor) of one layer kind, from rope_parameters
    {full_attention, sliding_attention} or rope_theta + rope_local_base_freq +
    rope_scaling (which concerns the global layers only)."""
    t = text_config(cfg_json)
    theta = t.get("rope_local_base_freq", 1e4) if local else \
        t.get("rope_theta", 1e6)
    factor = 1.0
    rs = t.get("rope_scaling")
    srcs = [None if local else rs,
            (t.get("rope_parameters") or {}).get(
                "sliding_attention" if local else "full_attention")]
    for d in srcs:
        if not d:
            continue
        theta = d.get("rope_theta", theta)
        if d.get("rope_type", d.get("type")) == "linear":
            factor = d["factor"]
    return float(theta), float(factor)


def rope_tables64(cfg_json: dict, max_seq: int, local: bool):
    """(cos, sin, angle): float64 (max_seq, hd/2); inv_freq_i =
    1 / (factor * theta^(2i/hd))."""
    hd = text_config(cfg_json)["head_dim"]
    theta, factor = rope_params(cfg_json, local)
    i = np.arange(hd // 2, dtype=np.float64)
    inv = 1.0 / (factor * np.power(theta, 2.0 * i / hd))
    a = np.arange(max_seq, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(a), np.sin(a), a


def rope_tables32(cfg_json: dict, max_seq: int, local: bool):
    """The same in the engine's order: the frequencies in double from the f32
    theta and factor, rounded to f32 once; the position product, cos and sin
    in f32."""
    f32 = np.float32
    hd = text_config(cfg_json)["head_dim"]
    theta, factor = rope_params(cfg_json, local)
    i = np.arange(hd // 2, dtype=np.float64)
    inv = (1.0 / (float(f32(factor)) * np.power(float(f32(theta)),
                                                2.0 * i / hd))).astype(f32)
    a = (np.arange(max_seq, dtype=f32)[:, None] * inv[None, :]).astype(f32)
    return np.cos(a).astype(f32), np.sin(a).astype(f32)


def gelu_tanh(g):
    g = g.astype(np.float32)
    return (0.5 * g * (1.0 + np.tanh(
        np.float32(math.sqrt(2.0 / math.pi)) *
        (g + np.float32(0.044715) * g * g * g)))).astype(np.float32)


class Gemma3Oracle(OracleModel):
    """t: {HF tensor name: array} with the "model." prefix.  defect: one of
    DEFECTS, or None.  act_bf16: round the activations to bf16 where the engine
    stores them, with its folded bf16 norm rows and bf16(sqrt(H)) embedding
    scale: the headroom estimate of tools/gen_golden_gemma3.py."""

    def __init__(self, cfg_json: dict, t: dict, max_seq: int, defect=None,
                 act_bf16=False):
        assert defect is None or defect in DEFECTS
        tc = text_config(cfg_json)
        self.tc, self.t, self.defect = tc, t, defect
        self.cfg = Config.from_json(dict(tc, tie_word_embeddings=True))
        self.kv = [None] * self.cfg.num_hidden_layers
        self.r = _bf16 if act_bf16 else (lambda a: a)
        self.act_bf16 = act_bf16
        self.local = layer_kinds(cfg_json)
        if defect == "all_global":
            self.local = [False] * len(self.local)
        if defect == "all_local":
            self.local = [True] * len(self.local)
        self.window = tc["sliding_window"]
        tabs = {}
        for loc in (False, True):
            j = cfg_json
            if defect == "linear_ignored" and not loc:
                theta, _ = rope_params(cfg_json, False)
                j = dict(tc, rope_parameters=None, rope_scaling=None,
                         rope_theta=theta)
            src = False if defect == "global_theta_all" else loc
            c, s, _ = rope_tables64(j, max_seq, src)
            tabs[loc] = (c.astype(np.float32), s.astype(np.float32))
        self.tabs = tabs
        qpas = tc["query_pre_attn_scalar"]
        self.scale = (self.cfg.hd if defect == "hd_scale" else qpas) ** -0.5

    # a norm row as the engine applies it: 1 + w (f32; bf16 under act_bf16)
    def nw(self, name, mul=1.0):
        w = self.t[name].astype(np.float32)
        if self.defect == "plain_w_norms":
            return w
        w = (np.float32(1.0) + w) * np.float32(mul)
        return _bf16(w) if self.act_bf16 else w

    def norm(self, x, name, mul=1.0):
        return self.r(rms_norm(x, self.nw(name, mul), self.cfg.rms_norm_eps))

    def attention(self, p, x, index_pos, li):
        cfg, r, t = self.cfg, self.r, self.t
        b, s, _ = x.shape
        hd, nh, nkv = cfg.hd, cfg.num_attention_heads, cfg.num_key_value_heads
        q = r(linear(x, t[p + "self_attn.q_proj.weight"])).reshape(b, s, nh, hd)
        k = r(linear(x, t[p + "self_attn.k_proj.weight"])).reshape(b, s, nkv, hd)
        v = r(linear(x, t[p + "self_attn.v_proj.weight"])).reshape(b, s, nkv, hd)
        # under act_bf16 the engine's q row carries the score-scale fold
        fold = math.sqrt(hd) * self.scale if self.act_bf16 else 1.0
        q = rms_norm(q, self.nw(p + "self_attn.q_norm.weight", fold),
                     cfg.rms_norm_eps).transpose(0, 2, 1, 3)
        k = rms_norm(k, self.nw(p + "self_attn.k_norm.weight"),
                     cfg.rms_norm_eps).transpose(0, 2, 1, 3)
        v = v.transpose(0, 2, 1, 3)
        loc = self.local[li]
        if not (loc and self.defect == "local_no_rope"):
            c, sn = self.tabs[loc]
            c, sn = c[index_pos:index_pos + s], sn[index_pos:index_pos + s]
            q, k = rope(q, c, sn), rope(k, c, sn)
        q, k = r(q), r(k)
        if self.kv[li] is not None:
            ck, cv = self.kv[li]
            k = np.concatenate([ck, k], axis=2)
            v = np.concatenate([cv, v], axis=2)
        self.kv[li] = (k, v)
        kv_len = k.shape[2]
        kr = np.repeat(k, nh // nkv, axis=1)
        vr = np.repeat(v, nh // nkv, axis=1)
        sc = hd ** -0.5 if self.act_bf16 else self.scale
        att = q @ kr.transpose(0, 1, 3, 2) * np.float32(sc)
        win = self.window if loc else None
        if s > 1 or win:
            att = np.where(causal_mask(s, kv_len, win)[None, None],
                           np.float32(-np.inf), att)
        y = r(softmax_lastdim(att) @ vr)
        y = y.transpose(0, 2, 1, 3).reshape(b, s, nh * hd)
        return linear(y, t[p + "self_attn.o_proj.weight"])

    def mlp(self, p, x):
        r, t = self.r, self.t
        gate = linear(x, t[p + "mlp.gate_proj.weight"])
        up = linear(x, t[p + "mlp.up_proj.weight"])
        if x.shape[1] > 1:      # prefill stores gate|up in bf16; decode fuses
            gate, up = r(gate), r(up)
        act = silu_mul(gate, up) if self.defect == "silu_gate" else \
            gelu_tanh(gate) * up.astype(np.float32)
        return linear(r(act), t[p + "mlp.down_proj.weight"])

    def block(self, i, x, index_pos):
        p, r = f"model.layers.{i}.", self.r
        post = self.defect != "no_post_norms"
        a = r(self.attention(p, self.norm(x, p + "input_layernorm.weight"),
                             index_pos, i))
        if post:
            a = self.norm(a, p + "post_attention_layernorm.weight")
        x = r(x + a)
        m = r(self.mlp(p, self.norm(x, p + "pre_feedforward_layernorm.weight")))
        if post:
            m = self.norm(m, p + "post_feedforward_layernorm.weight")
        return r(x + m)

    def embed(self, token_ids):
        e = self.t["model.embed_tokens.weight"]
        x = e[token_ids].astype(np.float32)
        if self.defect == "no_embed_scale":
            return x
        s = np.float32(math.sqrt(self.cfg.hidden_size))
        return self.r(x * (_bf16(s) if self.act_bf16 else s))

    def forward(self, token_ids, index_pos):
        x = self.embed(token_ids)
        for i in range(self.cfg.num_hidden_layers):
            x = self.block(i, x, index_pos)
        x = self.norm(x, "model.norm.weight")
        return linear(x[:, -1, :], self.t["model.embed_tokens.weight"])

    def hidden_forward(self, x, index_pos, lo, hi):
        for i in range(lo, hi):
            x = self.block(i, x, index_pos)
        return x


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def defect_moves(cfg_json, t, prompt, max_seq):
    """{defect: relative logits move on `prompt`} and the clean logits."""
    toks = np.asarray(prompt, dtype=np.int64)[None, :]
    base = Gemma3Oracle(cfg_json, t, max_seq).forward(toks, 0)[0]
    return {d: rel(Gemma3Oracle(cfg_json, t, max_seq, defect=d
                                ).forward(toks, 0)[0], base)
            for d in DEFECTS}, base


def fixture(golden_dir: str, name: str = "tiny_gemma3"):
    """(cfg_json, {tensor name: array}, npz) of the committed fixture."""
    z = np.load(os.path.join(golden_dir, f"{name}.npz"))
    with open(os.path.join(golden_dir, f"{name}.config.json")) as f:
        cfg_json = json.load(f)
    return cfg_json, {k[2:]: z[k] for k in z.files if k.startswith("w.")}, z
