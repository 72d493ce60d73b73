"""Reference for the head_dim-256 engine tests: the oracle's llama forward with
three attention defects a 256-wide head invites, and the bf16-activation
estimate.  tools/gen_golden_falcon3.py builds tests/golden/tiny_falcon3 so that
each defect moves the logits by at least four times the engine tests' 2e-2
gate; tests/test_hd256_ref.py checks that on the committed file."""
import numpy as np

from oracle import (Config, LayerWeights, ModelWeights, causal_mask, linear,
                    rope, softmax_lastdim)
from tests.phi3_ref import Phi3Oracle

# what a kernel written for hd 128 gets wrong at hd 256
ATTN_DEFECTS = (
    "score_low_half",    # the score summed over dims [0, 128) only
    "out_high_from_low",  # output dims [128, 256) taken from [0, 128)
    "scale_128",         # 1/sqrt(128) instead of 1/sqrt(256)
)


class Hd256Oracle(Phi3Oracle):
    """Phi3Oracle (full rotary here: a plain llama config) with an optional
    attention defect.  act_bf16 as there."""

    def __init__(self, cfg: Config, w: ModelWeights, cfg_json: dict,
                 max_seq: int, defect=None, act_bf16=False):
        assert defect is None or defect in ATTN_DEFECTS
        super().__init__(cfg, w, cfg_json, max_seq, None, act_bf16)
        self.attn_defect = defect

    def attention(self, lw: LayerWeights, x, index_pos, block_idx):
        cfg, r, defect = self.cfg, self.r, self.attn_defect
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
        q = r(rope(q, c, sn))
        k = r(rope(k, c, sn))
        if self.kv[block_idx] is not None:
            ck, cv = self.kv[block_idx]
            k = np.concatenate([ck, k], axis=2)
            v = np.concatenate([cv, v], axis=2)
        self.kv[block_idx] = (k, v)
        kv_len = k.shape[2]
        rep = nh // nkv
        kr = np.repeat(k, rep, axis=1)
        vr = np.repeat(v, rep, axis=1)
        qs = q
        if defect == "score_low_half":
            qs = q.copy()
            qs[..., hd // 2:] = 0
        scale = np.sqrt(hd / 2 if defect == "scale_128" else hd)
        att = qs @ kr.transpose(0, 1, 3, 2) / np.float32(scale)
        win = cfg.window_for(block_idx)
        if s > 1 or win:
            att = np.where(causal_mask(s, kv_len, win)[None, None],
                           np.float32(-np.inf), att)
        y = r(softmax_lastdim(att) @ vr)
        if defect == "out_high_from_low":
            y = np.concatenate([y[..., :hd // 2], y[..., :hd // 2]], axis=-1)
        y = y.transpose(0, 2, 1, 3).reshape(b, s, size_q)
        return linear(y, lw.o_proj)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def defect_moves(cfg, w, cfg_json, prompt, max_seq):
    """{defect: relative logits move on `prompt`} and the clean logits."""
    toks = np.asarray(prompt, dtype=np.int64)[None, :]
    base = Hd256Oracle(cfg, w, cfg_json, max_seq).forward(toks, 0)[0]
    return {d: rel(Hd256Oracle(cfg, w, cfg_json, max_seq, defect=d
                               ).forward(toks, 0)[0], base)
            for d in ATTN_DEFECTS}, base
