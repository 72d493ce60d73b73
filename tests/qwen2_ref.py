"""The oracle for qwen2 / qwen2.5: oracle.OracleModel with the additive bias of
the q, k and v projections (qwen2/config.rs:84 use_qkv_bias; the reference
loads it at attention.rs:95-104 and applies it in linear_forward(x, W, bias),
attention.rs:163).  Nothing else differs from the llama-shaped model.

Test infrastructure only, like oracle/ itself."""
import numpy as np

from oracle import (Config, LayerWeights, OracleModel, causal_mask, linear,
                    rope, softmax_lastdim)

BIAS_KEYS = ("q_proj", "k_proj", "v_proj")


class Qwen2Oracle(OracleModel):
    """biases: one fused (nh*hd + 2*nkv*hd,) f32 row per layer, q rows then k
    rows then v rows (the order of the fused qkv weight)."""

    def __init__(self, cfg: Config, w, biases):
        super().__init__(cfg, w)
        assert len(biases) == cfg.num_hidden_layers
        self.biases = [np.asarray(b, dtype=np.float32) for b in biases]

    def attention(self, lw: LayerWeights, x, index_pos, block_idx):
        cfg = self.cfg
        b, s, _ = x.shape
        hd, nh, nkv = cfg.hd, cfg.num_attention_heads, cfg.num_key_value_heads
        size_q, size_kv = nh * hd, nkv * hd
        qkv_w = np.concatenate([lw.q_proj, lw.k_proj, lw.v_proj], axis=0)
        # the one difference: the fused bias right after the qkv linear
        qkv = linear(x, qkv_w, self.biases[block_idx])
        q = qkv[..., :size_q].reshape(b, s, nh, hd).transpose(0, 2, 1, 3)
        k = qkv[..., size_q:size_q + size_kv].reshape(
            b, s, nkv, hd).transpose(0, 2, 1, 3)
        v = qkv[..., size_q + size_kv:].reshape(
            b, s, nkv, hd).transpose(0, 2, 1, 3)
        c = self.cos[index_pos:index_pos + s]
        sn = self.sin[index_pos:index_pos + s]
        q = rope(q, c, sn)
        k = rope(k, c, sn)
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
        y = softmax_lastdim(att) @ vr
        y = y.transpose(0, 2, 1, 3).reshape(b, s, size_q)
        return linear(y, lw.o_proj)


def bias_tensors(biases, cfg: Config, dtype=np.float32) -> dict:
    """The fused rows split into the checkpoint's three tensors per layer,
    `self_attn.{q,k,v}_proj.bias`."""
    sq = cfg.num_attention_heads * cfg.hd
    skv = cfg.num_key_value_heads * cfg.hd
    out = {}
    for i, b in enumerate(biases):
        p = f"model.layers.{i}.self_attn."
        out[p + "q_proj.bias"] = np.ascontiguousarray(b[:sq], dtype=dtype)
        out[p + "k_proj.bias"] = np.ascontiguousarray(b[sq:sq + skv],
                                                      dtype=dtype)
        out[p + "v_proj.bias"] = np.ascontiguousarray(b[sq + skv:],
                                                      dtype=dtype)
    return out


def fused_biases(tensors: dict, cfg: Config):
    """Inverse of bias_tensors, from a {name: array} mapping."""
    out = []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}.self_attn."
        out.append(np.concatenate([
            np.asarray(tensors[p + k + ".bias"], dtype=np.float32)
            for k in BIAS_KEYS]))
    return out


def random_biases(cfg: Config, seed: int, q_std=3.0, v_std=0.25):
    """q and k rows ~ N(0, q_std), v rows ~ N(0, v_std): real qwen2 q/k biases
    are large, and only a large one moves the logits when it is dropped (a
    constant added to every key barely changes a softmax)."""
    rng = np.random.default_rng(seed)
    sq = cfg.num_attention_heads * cfg.hd
    skv = cfg.num_key_value_heads * cfg.hd
    return [np.concatenate([rng.standard_normal(sq + skv) * q_std,
                            rng.standard_normal(skv) * v_std]
                           ).astype(np.float32)
            for _ in range(cfg.num_hidden_layers)]


def drop_one(biases, cfg: Config, which: str):
    """The biases with the q, k or v part zeroed in every layer."""
    sq = cfg.num_attention_heads * cfg.hd
    skv = cfg.num_key_value_heads * cfg.hd
    lo, hi = {"q": (0, sq), "k": (sq, sq + skv),
              "v": (sq + skv, sq + 2 * skv)}[which]
    out = [b.copy() for b in biases]
    for b in out:
        b[lo:hi] = 0
    return out
