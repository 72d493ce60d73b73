"""Host-side tests (no GPU): library loads + exports every declared symbol,
topology YAML parsing (range expressions, contiguity), bf16 helpers."""
import ctypes
import os
import re

import numpy as np
import pytest

import cake_amd
from cake_amd import CakeHipError, topology_node_range

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOPO = """\
# cake-style topology (sharding/topology.rs:134-169)
linux_server_1:
  host: 192.168.1.2:10128
  description: NVIDIA Titan X Pascal (12GB)
  layers:
    - model.layers.0-15
linux_server_2:
  host: 192.168.1.3:10128
  layers:
    - model.layers.16-31
odd_node:
  host: 192.168.1.4:10128
  layers:
    - model.layers.40
    - model.layers.42
single:
  host: 192.168.1.5:10128
  layers:
    - model.layers.7
"""


def test_library_loads_and_reports_gfx950():
    assert "gfx950" in cake_amd.build_info()


def test_header_symbols_all_exported():
    """Every cake_hip_* function declared in include/cake_hip.h must be an
    exported symbol of the built library (tier framing §3: the C-ABI library
    loads and exports every declared entry point)."""
    hdr = open(os.path.join(REPO, "include", "cake_hip.h")).read()
    names = set(re.findall(r"\b(cake_hip_\w+)\s*\(", hdr))
    assert len(names) >= 15
    for n in sorted(names):
        assert hasattr(cake_amd._lib, n), f"symbol {n} not exported"


def test_topology_range_expansion():
    # "model.layers.0-15" expands per topology.rs:142-166
    assert topology_node_range(TOPO, "linux_server_1") == (0, 16)
    assert topology_node_range(TOPO, "linux_server_2") == (16, 32)
    assert topology_node_range(TOPO, "single") == (7, 8)


def test_topology_rejects_noncontiguous():
    with pytest.raises(CakeHipError, match="contiguous"):
        topology_node_range(TOPO, "odd_node")


def test_topology_missing_node():
    with pytest.raises(CakeHipError, match="not in topology"):
        topology_node_range(TOPO, "nope")


def test_topology_invalid_range_order():
    bad = "n:\n  layers:\n    - model.layers.5-2\n"
    with pytest.raises(CakeHipError):
        topology_node_range(bad, "n")


def test_quantize_bf16_matches_rne():
    from tests.helpers import quantize_bf16
    import torch
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    ours = quantize_bf16(x)
    ref = torch.tensor(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(ours, ref)


def test_engine_requires_gpu_no_silent_fallback():
    """On a box with no GPU the engine must fail loudly, not fall back to
    CPU (tier framing §3)."""
    import os
    import torch
    # torch alone does not tell: once libcake_hip has initialised HIP in this
    # process (any GPU test that ran before), torch's own runtime reports no
    # device on a machine that has one.  /dev/kfd is the ROCm compute node.
    if torch.cuda.is_available() or os.path.exists("/dev/kfd"):
        pytest.skip("GPU present")
    with pytest.raises(CakeHipError):
        cake_amd.Engine(dict(
            model_type="llama", hidden_size=64, intermediate_size=128,
            vocab_size=128, num_hidden_layers=1, num_attention_heads=4,
            num_key_value_heads=2, head_dim=16), max_seq=32)


def test_engine_rejects_bad_config():
    # config parsing precedes any GPU call, so these are CPU-testable
    import json as _json
    with pytest.raises(_json.JSONDecodeError):
        cake_amd.Engine("not json at all {", max_seq=32)  # wrapper-side
    with pytest.raises(CakeHipError, match="missing required"):
        cake_amd.Engine(dict(model_type="llama", hidden_size=64,
                             num_hidden_layers=1), max_seq=32)


def _attn_args(nh=4, nkv=2, hd=128, max_seq=64, S=3):
    q = np.zeros((S, nh, hd), np.float32)
    kc = np.zeros((nkv, max_seq, hd), np.float32)
    vtc = np.zeros((nkv, hd, max_seq), np.float32)
    return q, kc, vtc


@pytest.mark.parametrize("kw,msg", [
    (dict(nh=3), "multiple of nkv"),
    (dict(hd=12), "hd 12"),
    (dict(hd=136), "hd 136"),
    (dict(max_seq=48), "max_seq 48"),
])
def test_attn_ops_reject_bad_geometry_without_gpu(kw, msg):
    """Argument checks precede every device call: each attention op entry
    names itself in the error, GPU or not."""
    q, kc, vtc = _attn_args(**kw)
    nh, nkv, hd = q.shape[1], kc.shape[0], q.shape[2]
    with pytest.raises(CakeHipError, match=f"op_attn_prefill.*{msg}"):
        cake_amd.op_attn_prefill(q, kc, kc, vtc, 0)
    with pytest.raises(CakeHipError, match=f"op_attn_decode.*{msg}"):
        cake_amd.op_attn_decode(q[0], kc, kc, 0)
    qkv = np.zeros((q.shape[0], (nh + 2 * nkv) * hd), np.float32)
    tab = np.zeros((kc.shape[1], hd // 2), np.float32)
    with pytest.raises(CakeHipError, match=f"op_kv_store.*{msg}"):
        cake_amd.op_kv_store(qkv, tab, tab, kc, kc, vtc, 0, nh, nkv)


def test_attn_ops_reject_bad_ranges_without_gpu():
    q, kc, vtc = _attn_args()
    with pytest.raises(CakeHipError, match="op_attn_prefill.*outside the cache"):
        cake_amd.op_attn_prefill(q, kc, kc, vtc, 62)
    with pytest.raises(CakeHipError, match="op_attn_decode.*outside the cache"):
        cake_amd.op_attn_decode(q[0], kc, kc, 64)
    for nchunk in (0, 65):
        with pytest.raises(CakeHipError, match="op_attn_decode.*nchunk"):
            cake_amd.op_attn_decode(q[0], kc, kc, 5, nchunk=nchunk)
    with pytest.raises(CakeHipError, match="op_attn_decode.*repeats"):
        cake_amd.op_attn_decode(q[0], kc, kc, 5, repeats=0)
    qkv = np.zeros((3, 8 * 128), np.float32)
    tab = np.zeros((64, 64), np.float32)
    with pytest.raises(CakeHipError, match="op_kv_store.*outside the cache"):
        cake_amd.op_kv_store(qkv, tab, tab, kc, kc, vtc, 62, 4, 2)
    with pytest.raises(CakeHipError, match="op_kv_store.*one row"):
        cake_amd.op_kv_store(qkv, tab, tab, kc, kc, vtc, 0, 4, 2, decode=True)


@pytest.mark.parametrize("hd,variant", [
    (128, (0, 0, 0, 0)),      # hd 128 never reaches the generic kernel
    (128, (1, 4, 0, 0)),      # v1 has no 4-wave form
    (128, (1, 8, 1, 0)),      # ... and no split
    (128, (2, 6, 0, 0)),
    (128, (2, 8, 1, 1)),      # split wins over deep in the dispatcher
    (128, (2, 4, 0, 3)),
    (64, (2, 8, 0, 0)),       # MFMA kernels are hd 128 only
])
def test_attn_prefill_rejects_inexpressible_variant_without_gpu(hd, variant):
    q, kc, vtc = _attn_args(hd=hd)
    with pytest.raises(CakeHipError, match="op_attn_prefill.*not dispatchable"):
        cake_amd.op_attn_prefill(q, kc, kc, vtc, 0, variant=variant)


def test_attention_dispatch_unchanged_for_bench_shapes():
    """launch_attn_prefill / launch_attn_decode choose their kernels through
    attn_prefill_policy / attn_decode_grid_y; restate the rules those
    functions had before they were split out and compare on every model and
    sequence length bench.py runs (prompt 128, matrix prefill 512, headline
    prefill 2048, the max_seq 4096 ceiling)."""
    from cake_amd.configs import MODELS
    env = lambda k, d: int(os.environ.get(k, d))
    pfv, nw_env = env("CAKE_PF_ATTN", 2), env("CAKE_PF_NW", 0)
    split_env, deep_env = env("CAKE_PF_SPLIT", 0), env("CAKE_PF_DEEP", 0)
    v2 = env("CAKE_ATTN_V2", 1) != 0
    for name, cfg in MODELS.items():
        nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
        hd = cfg.get("head_dim") or cfg["hidden_size"] // nh
        G = nh // nkv
        gy = 0
        if hd == 128 and v2:
            gy = nkv * (G // 4) if G >= 4 and G % 4 == 0 else \
                nkv if G in (1, 2) else 0
        for S in (1, 128, 512, 1024, 2048, 4096):
            got = cake_amd.attn_dispatch(S, nh, nkv, hd)
            nw4 = (nw_env == 4) if nw_env else (S + 255) // 256 * nh < 512
            # effective split: the wrapper passes the knob and the S >= 1024
            # rule on; the launcher applies them (and needs a workspace)
            split = split_env != 0 and S >= 1024
            got_split = bool(got["split"]) and S >= got["split_min_s"]
            deep = deep_env if (not split and deep_env in (1, 2)) else 0
            got_deep = got["deep"] if (not got_split
                                       and got["deep"] in (1, 2)) else 0
            assert (got["pfv"], got["nw"], got_split, got_deep,
                    got["decode_grid_y"]) == (
                        pfv, 4 if nw4 else 8, split, deep, gy), (name, S)
    if not any(k in os.environ for k in ("CAKE_PF_ATTN", "CAKE_PF_NW",
                                         "CAKE_PF_SPLIT", "CAKE_PF_DEEP")):
        # the defaults, spelled out for the flagship (nh 32): 128-row blocks
        # up to S = 3840, 256-row blocks from 16 * 32 = 512 grid blocks on
        d = cake_amd.attn_dispatch
        assert (d(2048, 32, 8, 128)["nw"], d(4096, 32, 8, 128)["nw"]) == (4, 8)
        assert d(2048, 32, 8, 128)["pfv"] == 2
        assert not d(2048, 32, 8, 128)["split"]
        assert d(2048, 32, 8, 128)["deep"] == 0
        assert d(1, 32, 8, 128)["decode_grid_y"] == 8
        assert d(1, 64, 8, 128)["decode_grid_y"] == 16


def test_engine_rejects_bad_layer_range():
    with pytest.raises(CakeHipError, match="layer range"):
        cake_amd.Engine(dict(
            model_type="llama", hidden_size=64, intermediate_size=128,
            vocab_size=128, num_hidden_layers=2, num_attention_heads=4,
            num_key_value_heads=2, head_dim=16), layer_lo=1, layer_hi=1)
