"""GPU engine tests (-m gpu) of the fp8 weight format: every family the engine
serves under fp8 (llama, QK-norm, qwen2 bias, both window forms, hd 64 and 128,
tied embeddings), the three decode norm routes, the K routes of the fp8 GEMV
(KB 1, KB 2 with a tail, the streaming kernel), graph replay, chunked prefill,
layer shards, init_random and the loader's fp8 branch.

Cases, reference and seeds are tests/fp8_cases.py; tests/test_fp8_ref.py shows
on the CPU that each defect these gates are for moves the gated quantity by at
least four times the gate, and that no greedy step of the reference is within
twice the gate of a tie, so ids are compared exactly.

Gates: prefill logits at GATE = 3e-2, the project's fp8 logits gate, and the
hidden states at the same value.  Every test prints what it observed (-s)."""
import contextlib
import json
import struct

import numpy as np
import pytest

import cake_amd
from tests import fp8_cases as fc
from tests.fp8_cases import GATE, GEN, rel_err

pytestmark = pytest.mark.gpu

ROUTES = {"default": {}, "fused": {"CAKE_FP8_SPLITNORM": "0"},
          "chain": {"CAKE_FP8_NORMCHAIN": "1"}}
EAGER = cake_amd.HAS_EMBED | cake_amd.HAS_HEAD
ALL = pytest.mark.parametrize("route", list(ROUTES))
EVERY = pytest.mark.parametrize("name", fc.NAMES)
MISSING_SCALE = "model.layers.1.self_attn.k_proj.weight_scale_inv"


def _save(tensors, path, dtypes=None):
    """Write a checkpoint; dtypes maps a tensor name to "BF16", "F16" or
    "F8_E4M3" (numpy has no bf16 or fp8: those go through torch)."""
    import torch
    from safetensors.torch import save_file
    tt = {k: torch.from_numpy(np.ascontiguousarray(v))
          for k, v in tensors.items()}
    for k, d in (dtypes or {}).items():
        tt[k] = (tt[k].view(torch.float8_e4m3fn) if d == "F8_E4M3" else
                 tt[k].to(torch.bfloat16 if d == "BF16" else torch.float16))
    save_file(tt, path)


def _save_by_hand(tensors, path, dtype_names):
    """The same file without a library: 8-byte header length, JSON header,
    data (for a dtype string the installed writer does not know)."""
    names = {"uint8": "U8", "float32": "F32"}
    header, blobs, off = {}, [], 0
    for k, v in tensors.items():
        raw = np.ascontiguousarray(v).tobytes()
        header[k] = dict(dtype=dtype_names.get(k, names[str(v.dtype)]),
                         shape=list(v.shape), data_offsets=[off, off + len(raw)])
        blobs.append(raw)
        off += len(raw)
    h = json.dumps(header).encode()
    h += b" " * (-len(h) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)) + h + b"".join(blobs))


@contextlib.contextmanager
def _engine(cfg_json, st=None, lo=0, hi=None, flags=None, seed=None):
    eng = cake_amd.Engine(json.dumps(cfg_json), lo, hi, flags=flags,
                          max_seq=fc.MAX_SEQ,
                          max_batch_tokens=fc.MAX_BATCH_TOKENS)
    try:
        if st is not None:
            eng.load_safetensors(st)
        if seed is not None:
            eng.init_random(seed=seed)
        yield eng
    finally:
        eng.close()


@pytest.fixture
def route_env(monkeypatch):
    """Selects a norm route: the engine reads the knobs when it is created."""
    def select(route):
        for k in ("CAKE_FP8_SPLITNORM", "CAKE_FP8_NORMCHAIN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in ROUTES[route].items():
            monkeypatch.setenv(k, v)
    return select


@pytest.fixture
def ckpt(tmp_path):
    def write(name):
        st = str(tmp_path / f"{name}.safetensors")
        _save(fc.case(name)["tensors"], st)
        return st
    return write


def _greedy(eng, prompt, n):
    return [int(eng.prefill(prompt))] + [int(t) for t in eng.decode(n - 1)]


def _hidden(eng, name, steps=fc.HID_STEPS):
    """The engine's side of fp8_cases.hidden_outputs."""
    x12, xs = fc.hidden_inputs(name)
    out = [eng.forward_hidden(x12, 0)]
    for i in range(steps):
        out.append(eng.forward_hidden(xs[i][None], fc.HID_ROWS + i))
    return out


def test_configs_reach_the_routes_they_are_named_for():
    """By the engine's own predicates (host only)."""
    d = {n: cake_amd.decode_dispatch(j) for n, j in fc.CONFIGS.items()}
    for n in fc.NAMES:
        assert d[n]["qkv"][0] == "gemv_fp8" and d[n]["gateup"][0] == "gateup_fp8"
    assert d["llama_hd64"]["down"] == ("gemv_fp8", 4, 1)
    assert d["wide_mlp"]["down"] == ("gemv_fp8_stream", 4, 0)
    assert d["wide_hidden"]["qkv"][2] == d["wide_hidden"]["gateup"][2] == 2
    per_head = {n: cake_amd.attn_dispatch(
        1, j["num_attention_heads"], j["num_key_value_heads"],
        j["head_dim"])["decode_grid_y"] == 0 for n, j in fc.CONFIGS.items()}
    assert per_head["llama_hd64"] and per_head["qwen2_hd64"]
    assert not per_head["mistral_hd128"] and not per_head["qwen3_hd128"]


# ---- 1-4: every config on every route -------------------------------------------
@EVERY
@ALL
def test_prefill_logits_vs_reference(name, route, route_env, ckpt):
    c = fc.case(name)
    route_env(route)
    with _engine(c["cfg_json"], ckpt(name)) as eng:
        _, logits = eng.prefill(c["prompt"], want_logits=True)
    r = rel_err(logits, c["logits"])
    print(f"fp8 {name} {route}: prefill logits rel err {r:.3e}")
    assert r < GATE, f"prefill logits rel err {r}"


@EVERY
@ALL
def test_decode_hidden_vs_reference(name, route, route_env, ckpt):
    """12 rows at position 0, then single rows at 12..19 (the decode kernels,
    across the window of 16; on the chain route layer 0 takes the fall-back
    without a published scale and layer 1 reads the chain)."""
    c = fc.case(name)
    route_env(route)
    with _engine(c["cfg_json"], ckpt(name)) as eng:
        got = _hidden(eng, name)
    errs = [rel_err(g, w) for g, w in zip(got, c["hidden"])]
    print(f"fp8 {name} {route}: hidden rel err prefill {errs[0]:.3e} "
          f"decode max {max(errs[1:]):.3e}")
    for i, r in enumerate(errs):
        assert r < GATE, f"hidden output {i} rel err {r}"


@EVERY
@ALL
def test_greedy_ids_equal_the_reference(name, route, route_env, ckpt):
    c = fc.case(name)
    route_env(route)
    with _engine(c["cfg_json"], ckpt(name)) as eng:       # USE_GRAPH
        got = _greedy(eng, c["prompt"], GEN)
    assert got == c["ids"], (got, c["ids"], c["gaps"])


@EVERY
@ALL
def test_graph_and_eager_agree(name, route, route_env, ckpt):
    c = fc.case(name)
    route_env(route)
    st = ckpt(name)
    with _engine(c["cfg_json"], st) as g, \
            _engine(c["cfg_json"], st, flags=EAGER) as e:
        ids_g = _greedy(g, c["prompt"], GEN)
        ids_e = _greedy(e, c["prompt"], GEN)
        assert ids_e == c["ids"], (ids_e, c["ids"])
        assert ids_g == ids_e, "graph replay and eager decode disagree"
        # on: the replayed graph reuses the chain's counters step after step
        more_g = [int(t) for t in g.decode(GEN)]
        more_e = [int(t) for t in e.decode(GEN)]
    assert more_g == more_e, "graph and eager part after 8 ids"


# ---- 5: chunked prefill + append -------------------------------------------------
@pytest.mark.parametrize("name", ["qwen3_hd64_swa", "qwen2_hd64"])
def test_chunked_prefill_and_append(name, route_env, ckpt):
    c = fc.case(name)
    route_env("default")
    st = ckpt(name)
    with _engine(c["cfg_json"], st) as whole, \
            _engine(c["cfg_json"], st) as parts:
        one_shot = _greedy(whole, c["prompt"], 5)
        parts.prefill(c["prompt"][:25])
        first, logits = parts.prefill(c["prompt"][25:], want_logits=True)
        appended = [int(first)] + [int(t) for t in parts.decode(4)]
    r = rel_err(logits, c["logits"])
    print(f"fp8 {name}: 25 + 15 prefill logits rel err {r:.3e}")
    assert r < GATE, f"appended prefill logits rel err {r}"
    assert appended == one_shot


# ---- 6: layer shards -------------------------------------------------------------
@pytest.mark.parametrize("name", ["qwen3_hd128", "qwen2_hd64"])
@pytest.mark.parametrize("route", ["default", "chain"])
def test_two_shards_vs_reference_and_monolithic(name, route, route_env, ckpt):
    c = fc.case(name)
    route_env(route)
    st = ckpt(name)
    x12, xs = fc.hidden_inputs(name)
    with _engine(c["cfg_json"], st) as mono, \
            _engine(c["cfg_json"], st, 0, 1, flags=0) as lo, \
            _engine(c["cfg_json"], st, 1, 2, flags=0) as hi:
        worst = [0.0, 0.0]
        steps = [(x12, 0)] + [(xs[i][None], fc.HID_ROWS + i) for i in range(4)]
        for i, (x, pos) in enumerate(steps):
            whole = mono.forward_hidden(x, pos)
            chained = hi.forward_hidden(lo.forward_hidden(x, pos), pos)
            rr, rm = rel_err(chained, c["hidden"][i]), rel_err(chained, whole)
            worst = [max(worst[0], rr), max(worst[1], rm)]
            assert rr < GATE, f"step {i}: shards vs reference {rr}"
            assert rm < GATE, f"step {i}: shards vs monolithic {rm}"
    print(f"fp8 {name} {route}: two shards rel err vs reference "
          f"{worst[0]:.3e}, vs monolithic {worst[1]:.3e}")


# ---- 7: init_random --------------------------------------------------------------
@pytest.mark.parametrize("name", ["qwen3_hd128", "qwen2_hd64"])
def test_init_random(name, route_env):
    c = fc.case(name)
    route_env("default")
    j, prompt = c["cfg_json"], c["prompt"]
    x12, _ = fc.hidden_inputs(name)
    with _engine(j, seed=1234) as a, _engine(j, seed=1234) as b, \
            _engine(j, seed=1234, flags=EAGER) as e:
        _, logits = a.prefill(prompt, want_logits=True)
        assert np.isfinite(logits).all()
        a.reset()
        ids = _greedy(a, prompt, GEN)
        assert ids == _greedy(b, prompt, GEN), "one seed, two engines"
        assert ids == _greedy(e, prompt, GEN), "graph vs eager"
        assert all(0 <= t < j["vocab_size"] for t in ids)
        a.reset()
        whole = a.forward_hidden(x12, 0)
    # salts go by layer identity: a shard holds the monolithic engine's layers
    with _engine(j, lo=0, hi=1, flags=0, seed=1234) as lo, \
            _engine(j, lo=1, hi=2, flags=0, seed=1234) as hi:
        chained = hi.forward_hidden(lo.forward_hidden(x12, 0), 0)
    r = rel_err(chained, whole)
    print(f"fp8 {name}: init_random two shards vs monolithic {r:.3e}")
    assert np.isfinite(whole).all() and r < GATE


# ---- 8: the loader's fp8 branch --------------------------------------------------
LOADER = "llama_hd64"


@pytest.fixture(scope="module")
def exact_model():
    """llama_hd64 with bf16-exact (so f16-exact) scales: do not modify."""
    j = fc.CONFIGS[LOADER]
    tensors, ref = fc.build_model(j, fc.MODEL_SEED[LOADER], exact_scales=True)
    prompt = fc.prompt_of(LOADER)
    return j, tensors, prompt, fc.prefill_logits(ref, prompt)


def test_loader_scale_and_weight_dtypes(exact_model, tmp_path):
    j, tensors, prompt, want = exact_model
    scales = [k for k in tensors if k.endswith(".weight_scale_inv")]
    weights = [k[:-len("_scale_inv")] for k in scales]
    for k in scales:                    # the premise: nothing is rounded
        assert np.array_equal(tensors[k].astype(np.float16).astype(np.float32),
                              tensors[k])
    ids = {}
    for kind, dtypes in (("F32", {}),
                         ("BF16", {k: "BF16" for k in scales}),
                         ("F16", {k: "F16" for k in scales}),
                         ("F8_E4M3", {k: "F8_E4M3" for k in weights})):
        st = str(tmp_path / f"{kind}.safetensors")
        try:
            _save(tensors, st, dtypes)
        except Exception:               # a writer without float8_e4m3fn
            assert kind == "F8_E4M3"
            _save_by_hand(tensors, st, dtypes)
        with open(st, "rb") as f:
            n, = struct.unpack("<Q", f.read(8))
            header = json.loads(f.read(n))
        for k, d in dtypes.items():
            assert header[k]["dtype"] == d
        with _engine(j, st) as eng:
            _, logits = eng.prefill(prompt, want_logits=True)
            eng.reset()
            ids[kind] = _greedy(eng, prompt, GEN)
        r = rel_err(logits, want)
        print(f"fp8 loader {kind}: prefill logits rel err {r:.3e}")
        assert r < GATE, f"{kind}: prefill logits rel err {r}"
    for kind in ids:
        assert ids[kind] == ids["F32"], (kind, ids)


def test_loader_refuses_bad_checkpoints(exact_model, tmp_path):
    j, tensors, _, _ = exact_model
    missing = {k: v for k, v in tensors.items() if k != MISSING_SCALE}
    # scales of a checkpoint quantized in 64 x 64 blocks: four times as many
    fine = {k: (np.repeat(np.repeat(v, 2, axis=0), 2, axis=1)
                if k.endswith(".weight_scale_inv") else v)
            for k, v in tensors.items()}
    q = "model.layers.0.self_attn.q_proj.weight"
    wide = dict(tensors)
    wide[q] = np.zeros(tensors[q].shape, dtype=np.float32)
    for what, t, dtypes, msg in (
            ("missing scale", missing, {}, MISSING_SCALE.replace(".", r"\.")),
            ("64 x 64 scales", fine, {}, "scale_inv shape mismatch"),
            ("bf16 weight", wide, {q: "BF16"}, "expected F8_E4M3/U8 tensor, "
                                               "got BF16")):
        st = str(tmp_path / "bad.safetensors")
        _save(t, st, dtypes)
        with _engine(j) as eng:
            with pytest.raises(cake_amd.CakeHipError, match=msg):
                eng.load_safetensors(st)


@pytest.mark.parametrize("block,shown", [([64, 64], r"\[64, 64\]"),
                                         ([128, 64], r"\[128, 64\]"),
                                         ([128], r"\[128\]"),
                                         (128, "128")])
def test_create_refuses_other_block_sizes(block, shown):
    j = json.loads(json.dumps(fc.CONFIGS[LOADER]))
    j["quantization_config"]["weight_block_size"] = block
    with pytest.raises(cake_amd.CakeHipError,
                       match="weight_block_size " + shown):
        cake_amd.Engine(json.dumps(j), max_seq=64, max_batch_tokens=32)


def test_create_accepts_an_absent_block_size_and_refuses_phi3():
    j = json.loads(json.dumps(fc.CONFIGS[LOADER]))
    del j["quantization_config"]["weight_block_size"]
    with _engine(j):
        pass
    j["model_type"] = "phi3"
    with pytest.raises(cake_amd.CakeHipError, match="phi3"):
        cake_amd.Engine(json.dumps(j), max_seq=64, max_batch_tokens=32)
