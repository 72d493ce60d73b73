"""The oracle for phi3 (Phi-3 / Phi-4-mini / Phi-4, phi4/ in the reference):
oracle.OracleModel with three changes.

  * the rope turns only the first rd = int(hd * partial_rotary_factor) dims of
    each q and k head (phi4/attention.rs:59-66, 86); the rest pass through;
  * the cos / sin tables come from `rope_tables64`, a float64 restatement of
    the engine's table rule: plain or LongRoPE frequencies, the attention
    factor, and the ONE list chosen by the engine's max_seq (HF transformers'
    _compute_longrope_parameters, with the per-engine instead of per-call list
    choice);
  * the checkpoint's fused tensors are split for the oracle (`split_fused`) and
    fused for the engine (`fused_tensors`).

Test infrastructure only, like oracle/ itself."""
import math

import numpy as np

from oracle import (Config, LayerWeights, ModelWeights, OracleModel,
                    causal_mask, linear, rms_norm, silu_mul, softmax_lastdim)

# table defects the tests must be able to see (rope_tables64 / Phi3Oracle)
ROPE_DEFECTS = ("full_rotation", "attention_factor_1", "short_factors_1",
                "short_list")


def rope_params(cfg_json: dict) -> dict:
    """The rotary fields of a config.json, in either spelling: top-level
    partial_rotary_factor / original_max_position_embeddings with rope_scaling
    {type}, or rope_parameters {rope_type, partial_rotary_factor, ...}."""
    nh = cfg_json["num_attention_heads"]
    hd = cfg_json.get("head_dim") or cfg_json["hidden_size"] // nh
    rp = cfg_json.get("rope_parameters") or {}
    prf = cfg_json.get("partial_rotary_factor",
                       rp.get("partial_rotary_factor", 1.0))
    theta = cfg_json.get("rope_theta", 1e6 if cfg_json.get("model_type") in
                         ("phi3", "qwen2") else 10000.0)
    out = dict(hd=hd, rd=int(np.float32(hd) * np.float32(prf)), theta=theta,
               max_pos=cfg_json.get("max_position_embeddings", 4096),
               longrope=None)
    for d in (cfg_json.get("rope_scaling"), rp):
        if d and d.get("rope_type", d.get("type")) in ("longrope", "su"):
            out["longrope"] = dict(
                short=list(d["short_factor"]), long=list(d["long_factor"]),
                orig=d.get("original_max_position_embeddings",
                           cfg_json.get("original_max_position_embeddings")),
                factor=d.get("factor"),
                attention_factor=d.get("attention_factor"))
            break
    return out


def rope_tables64(cfg_json: dict, max_seq: int, defect=None):
    """(cos, sin, angle, m): float64 (max_seq, rd/2) tables, the angles
    pos * inv_freq they are the cosine / sine of, and the attention factor.

    inv_freq_i = 1 / (f_i * theta^(2i/rd)), f = long_factor if max_seq >
    original_max_position_embeddings else short_factor (f = 1 without
    LongRoPE); m = attention_factor, or with s = factor or max_pos / original:
    1 if s <= 1 else sqrt(1 + ln s / ln original).

    defect (one of ROPE_DEFECTS) builds a WRONG table on purpose:
      full_rotation       rd = hd (partial_rotary_factor ignored; the factor
                          lists are padded with their last entry)
      attention_factor_1  m = 1
      short_factors_1     every short factor 1
      short_list          the short list whatever max_seq is"""
    assert defect is None or defect in ROPE_DEFECTS
    p = rope_params(cfg_json)
    rd = p["hd"] if defect == "full_rotation" else p["rd"]
    half = rd // 2
    i = np.arange(half, dtype=np.float64)
    f = np.ones(half)
    m = 1.0
    lr = p["longrope"]
    if lr is not None:
        orig = float(lr["orig"])
        use_long = max_seq > orig and defect != "short_list"
        lst = list(lr["long"] if use_long else lr["short"])
        if defect == "short_factors_1" and not use_long:
            lst = [1.0] * len(lst)
        lst = lst + [lst[-1]] * (half - len(lst))
        f = np.array(lst, dtype=np.float64)
        if lr["attention_factor"] is not None:
            m = float(lr["attention_factor"])
        else:
            s = lr["factor"] if lr["factor"] is not None else \
                p["max_pos"] / orig
            m = 1.0 if s <= 1.0 else math.sqrt(1.0 + math.log(s) /
                                               math.log(orig))
        if defect == "attention_factor_1":
            m = 1.0
    inv = 1.0 / (f * np.power(float(p["theta"]), 2.0 * i / rd))
    a = np.arange(max_seq, dtype=np.float64)[:, None] * inv[None, :]
    return m * np.cos(a), m * np.sin(a), a, m


def rope_tables32(cfg_json: dict, max_seq: int):
    """The LongRoPE rule in numpy float32 arithmetic, in the engine's order:
    the frequencies are computed in double and rounded to f32 once (an f32
    exponent 2i/rd alone costs ln(theta) 2^-24 relative), then the position
    product, cos / sin and the product with m are f32."""
    p = rope_params(cfg_json)
    rd, half = p["rd"], p["rd"] // 2
    f32 = np.float32
    i = np.arange(half, dtype=np.float64)
    base = np.power(float(f32(p["theta"])), 2.0 * i / rd)
    m = f32(1)
    lr = p["longrope"]
    if lr is None:
        inv = (1.0 / base).astype(f32)
    else:
        orig = f32(lr["orig"])
        lst = lr["long"] if f32(max_seq) > orig else lr["short"]
        inv = (1.0 / (np.array(lst, dtype=f32).astype(np.float64) * base)
               ).astype(f32)
        if lr["attention_factor"] is not None:
            m = f32(lr["attention_factor"])
        else:
            s = f32(lr["factor"]) if lr["factor"] is not None else \
                f32(p["max_pos"]) / orig
            m = f32(1) if s <= 1 else np.sqrt(
                f32(1) + np.log(s) / np.log(orig)).astype(f32)
    a = (np.arange(max_seq, dtype=f32)[:, None] * inv[None, :]).astype(f32)
    return (m * np.cos(a)).astype(f32), (m * np.sin(a)).astype(f32)


def partial_rope(x, cos, sin, rd):
    """HF half-rotation over x[..., :rd]; x[..., rd:] passes through.
    x (B, H, S, D); cos / sin (S, rd/2)."""
    half = rd // 2
    x1, x2, rest = x[..., :half], x[..., half:rd], x[..., rd:]
    c, s = cos[None, None], sin[None, None]
    return np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s, rest], axis=-1)


def _bf16(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


class Phi3Oracle(OracleModel):
    """max_seq: the engine's cache capacity (it picks the LongRoPE list).
    defect: one of ROPE_DEFECTS, or None.  act_bf16: round the activations to
    bf16 where the engine stores them (norm outputs, the qkv rows, the roped q
    and k, the attention output, the residual stream, the SwiGLU product) —
    the headroom estimate of tools/gen_golden_phi3.py."""

    def __init__(self, cfg: Config, w: ModelWeights, cfg_json: dict,
                 max_seq: int, defect=None, act_bf16=False):
        super().__init__(cfg, w)
        c, s, _, _ = rope_tables64(cfg_json, max_seq, defect)
        self.cos, self.sin = c.astype(np.float32), s.astype(np.float32)
        self.rd = 2 * c.shape[1]
        self.r = _bf16 if act_bf16 else (lambda a: a)

    def attention(self, lw: LayerWeights, x, index_pos, block_idx):
        cfg, r = self.cfg, self.r
        b, s, _ = x.shape
        hd, nh, nkv = cfg.hd, cfg.num_attention_heads, cfg.num_key_value_heads
        size_q, size_kv = nh * hd, nkv * hd
        qkv_w = np.concatenate([lw.q_proj, lw.k_proj, lw.v_proj], axis=0)
        qkv = r(linear(x, qkv_w))
        q = qkv[..., :size_q].reshape(b, s, nh, hd).transpose(0, 2, 1, 3)
        k = qkv[..., size_q:size_q + size_kv].reshape(
            b, s, nkv, hd).transpose(0, 2, 1, 3)
        v = qkv[..., size_q + size_kv:].reshape(
            b, s, nkv, hd).transpose(0, 2, 1, 3)
        c = self.cos[index_pos:index_pos + s]
        sn = self.sin[index_pos:index_pos + s]
        # the one difference: only the first rd dims rotate
        q = r(partial_rope(q, c, sn, self.rd))
        k = r(partial_rope(k, c, sn, self.rd))
        if self.kv[block_idx] is not None:
            ck, cv = self.kv[block_idx]
            k = np.concatenate([ck, k], axis=2)
            v = np.concatenate([cv, v], axis=2)
        self.kv[block_idx] = (k, v)
        kv_len = k.shape[2]
        rep = nh // nkv
        kr = np.repeat(k, rep, axis=1)
        vr = np.repeat(v, rep, axis=1)
        att = q @ kr.transpose(0, 1, 3, 2) / np.float32(np.sqrt(hd))
        win = cfg.window_for(block_idx)
        if s > 1 or win:
            att = np.where(causal_mask(s, kv_len, win)[None, None],
                           np.float32(-np.inf), att)
        y = r(softmax_lastdim(att) @ vr)
        y = y.transpose(0, 2, 1, 3).reshape(b, s, size_q)
        return linear(y, lw.o_proj)

    def mlp(self, lw: LayerWeights, x):
        r = self.r
        gate = r(linear(x, lw.gate_proj))
        up = r(linear(x, lw.up_proj))
        return linear(r(silu_mul(gate, up)), lw.down_proj)

    def block(self, i, x, index_pos):
        lw, r, eps = self.w.layers[i], self.r, self.cfg.rms_norm_eps
        h = r(rms_norm(x, lw.input_layernorm, eps))
        x = r(x + self.attention(lw, h, index_pos, i))
        h = r(rms_norm(x, lw.post_attention_layernorm, eps))
        return r(x + self.mlp(lw, h))

    def forward(self, token_ids, index_pos):
        x = self.w.embed_tokens[token_ids].astype(np.float32)
        for i in range(self.cfg.num_hidden_layers):
            x = self.block(i, x, index_pos)
        x = self.r(rms_norm(x, self.w.norm, self.cfg.rms_norm_eps))
        return linear(x[:, -1, :], self.w.lm_head)


def fused_tensors(flat: dict, cfg: Config) -> dict:
    """A split-name {tensor: array} mapping (tests/helpers.flatten) in the phi3
    checkpoint's names: self_attn.qkv_proj.weight = q|k|v rows and
    mlp.gate_up_proj.weight = gate rows, then up rows."""
    out = {k: v for k, v in flat.items()
           if not any(s in k for s in ("q_proj", "k_proj", "v_proj",
                                       "gate_proj", "up_proj"))}
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        out[p + "self_attn.qkv_proj.weight"] = np.concatenate(
            [flat[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], axis=0)
        out[p + "mlp.gate_up_proj.weight"] = np.concatenate(
            [flat[p + f"mlp.{n}_proj.weight"] for n in ("gate", "up")], axis=0)
    return out


def split_fused(t: dict, cfg: Config) -> ModelWeights:
    """Inverse of fused_tensors, into the oracle's containers."""
    sq = cfg.num_attention_heads * cfg.hd
    skv = cfg.num_key_value_heads * cfg.hd
    I = cfg.intermediate_size
    layers = []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        qkv = t[p + "self_attn.qkv_proj.weight"]
        gu = t[p + "mlp.gate_up_proj.weight"]
        layers.append(LayerWeights(
            input_layernorm=t[p + "input_layernorm.weight"],
            post_attention_layernorm=t[p + "post_attention_layernorm.weight"],
            q_proj=qkv[:sq], k_proj=qkv[sq:sq + skv], v_proj=qkv[sq + skv:],
            o_proj=t[p + "self_attn.o_proj.weight"],
            gate_proj=gu[:I], up_proj=gu[I:],
            down_proj=t[p + "mlp.down_proj.weight"]))
    embed = t["model.embed_tokens.weight"]
    return ModelWeights(
        embed_tokens=embed, norm=t["model.norm.weight"],
        lm_head=embed if cfg.tie_word_embeddings else t["lm_head.weight"],
        layers=layers)


def fixture(golden_dir: str, name: str = "tiny_phi3"):
    """(cfg_json, Config, ModelWeights, npz, fused tensors) of the committed
    phi3 fixture, whose npz holds the checkpoint's own (fused) tensors."""
    import json
    import os
    z = np.load(os.path.join(golden_dir, f"{name}.npz"))
    with open(os.path.join(golden_dir, f"{name}.config.json")) as f:
        cfg_json = json.load(f)
    cfg = Config.from_json(cfg_json)
    t = {k[2:]: z[k] for k in z.files if k.startswith("w.")}
    return cfg_json, cfg, split_fused(t, cfg), z, t
