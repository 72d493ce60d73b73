"""GPU tests (-m gpu) of k_attn_prefill_mfma_n, the MFMA prefill attention at
head_dim 64 and 96: the op against the float64 reference by the procedure of
tests/test_attn_ops_gpu.py (four input families, invisible slots zeroed and at
+-2^60 bit-identical, |got - ref| <= TOL_MFMA * A + ABS_EPS element-wise), and
the engine against the quantized oracle."""
import json
import os
import tempfile

import numpy as np
import pytest

import cake_amd
from oracle import Config, random_weights
from tests.attn_cases import (ABS_EPS, FAMILIES, STALE, TOL_MFMA, make_inputs,
                              set_stale)
from tests.attn_ref import attn_ref
from tests.helpers import weights_to_safetensors
from tests.test_gpu_parity import quantized_oracle, rel_err

pytestmark = pytest.mark.gpu

PF_MFMA_N = (1, 4, 0, 0)
# (nh, nkv, S, pos0, window, max_seq): the smallest shapes that cross the
# kernel's 64-key stage, 32-row wave and 128-row block boundaries
CASES = [
    (4, 2, 1, 0, 1, 32),        # one row, one key, cache shorter than a stage
    (2, 2, 31, 1, 0, 32),       # MHA; the last sub-tile ends the cache
    (4, 2, 33, 45, 40, 96),     # wave boundary, window start inside a
                                # sub-tile, the last stage overhangs the cache
    (2, 1, 32, 64, 32, 96),     # pos0 + S == max_seq, window == sub-tile
    (14, 2, 129, 64, 33, 224),  # G = 7; second block holds one row
    (2, 1, 257, 0, 0, 288),     # three blocks in reversed order, 9 sub-tiles
    (8, 1, 65, 63, 0, 128),     # first query at the last position of a stage
]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("hd", [64, 96])
def test_prefill_mfma_n(hd, case):
    nh, nkv, S, pos0, window, max_seq = case
    fails = []
    for fam in FAMILIES:
        q, kc, vc = make_inputs(fam, nh, nkv, hd, max_seq, S, pos0, window)
        ref, A = attn_ref(q, kc, vc, pos0, window)
        outs = []
        for fill in (0, STALE):
            k, v, vt = set_stale(kc, vc, 0, pos0 + S, fill)
            outs.append(cake_amd.op_attn_prefill(q, k, v, vt, pos0, window,
                                                 PF_MFMA_N))
        if not np.array_equal(_bits(outs[0]), _bits(outs[1])):
            fails.append(f"{fam}: output depends on stale slots >= {pos0 + S}")
        ratio = np.abs(outs[0] - ref) / (TOL_MFMA * A + ABS_EPS)
        worst = np.inf if np.isnan(outs[0]).any() else float(np.max(ratio))
        print(f"hd {hd} {case} {fam}: worst err/(tol*A) = {worst:.3f}")
        if not worst <= 1.0:
            i = np.unravel_index(np.argmax(ratio), ratio.shape)
            fails.append(f"{fam}: err/(tol*A) = {worst:.3f} at {i} "
                         f"(got {outs[0][i]:.6g}, ref {ref[i]:.6g})")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("hd", [64, 96])
def test_engine_prefill_parity(hd):
    """Two-layer llama at this head dim: prefill logits against the quantized
    oracle on ragged S, a chunked prefill (pos0 > 0) against the single-chunk
    one, and a greedy continuation after a prompt that ends mid-stage."""
    cfg_json = dict(
        model_type="llama", hidden_size=256, intermediate_size=512,
        vocab_size=512, num_hidden_layers=2, num_attention_heads=4,
        num_key_value_heads=2, head_dim=hd, rms_norm_eps=1e-5,
        rope_theta=500000.0, max_position_embeddings=1024,
        tie_word_embeddings=False)
    cfg = Config.from_json(cfg_json)
    w = random_weights(cfg, seed=23 + hd)
    oracle = quantized_oracle(cfg, w)
    assert cake_amd.attn_dispatch(33, 4, 2, hd)["pfv"] == 1
    with tempfile.TemporaryDirectory() as td:
        st = os.path.join(td, "m.safetensors")
        weights_to_safetensors(w, cfg, st)
        eng = cake_amd.Engine(json.dumps(cfg_json), max_seq=352,
                              max_batch_tokens=512)
        small = cake_amd.Engine(json.dumps(cfg_json), max_seq=352,
                                max_batch_tokens=48)
        try:
            eng.load_safetensors(st)
            small.load_safetensors(st)
            rng = np.random.default_rng(3)
            for S in (1, 33, 129, 300):
                prompt = rng.integers(0, cfg.vocab_size,
                                      size=S).astype(np.uint32)
                oracle.reset()
                ref = oracle.forward(prompt[None, :].astype(np.int64), 0)[0]
                eng.reset()
                _, logits = eng.prefill(prompt, want_logits=True)
                r = rel_err(logits, ref)
                print(f"hd {hd} S={S}: prefill logits rel err {r:.3e}")
                assert r < 2e-2, f"S={S}: prefill logits rel err {r}"
            # the 300-token prompt again in chunks of 48: pos0 = 48 .. 288
            _, chunked = small.prefill(prompt, want_logits=True)
            r = rel_err(chunked, logits)
            print(f"hd {hd}: chunked vs single-chunk rel err {r:.3e}")
            assert r < 2e-2, f"chunked != single-chunk: {r}"
            prompt = rng.integers(0, cfg.vocab_size, size=45).astype(np.uint32)
            oracle.reset()
            ref_toks = oracle.generate_greedy(list(prompt), 5)
            eng.reset()
            got = [eng.prefill(prompt)] + list(eng.decode(4))
            assert sum(a == b for a, b in zip(got, ref_toks)) >= 4, (
                got, ref_toks)
        finally:
            eng.close()
            small.close()
