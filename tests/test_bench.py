"""bench.py command-line contract: a plain run times only the headline
decode steps (every other leg sits behind --full) and --dump-outputs writes
the token ids the timed decode call returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")

FULL_ONLY_KEYS = ("prefill_tok_s", "prefill_roofline", "roofline",
                  "cpu_baseline", "matrix")


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], cwd=REPO,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout
    assert "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_timed_tokens(tmp_path):
    steps = 5
    out_dir = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps),
         "--warmup", "2", "--model", "qwen3-0.6b", "--max-seq", "256",
         "--dump-outputs", str(out_dir)],
        cwd=REPO, capture_output=True, text=True, timeout=120)
    sys.stderr.write(r.stderr[-2000:])
    assert r.returncode == 0
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, "exactly one JSON result line on stdout"
    res = json.loads(lines[0])
    assert res["metric"] == "decode tok/s" and res["unit"] == "tok/s"
    assert res["higher_is_better"] is True
    assert res["dtype"] == "bf16"
    assert res["steps"] == steps
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region
    assert res["value"] == pytest.approx(1000.0 / res["ms_per_step"],
                                         rel=1e-2)
    for k in FULL_ONLY_KEYS:
        assert res[k] is None, f"{k} must only be measured with --full"
    assert sorted(os.listdir(out_dir)) == ["tokens.npy"]
    toks = np.load(out_dir / "tokens.npy")
    assert toks.dtype == np.float64 and toks.shape == (steps,)
    assert np.all(toks == np.floor(toks))
    assert np.all((toks >= 0) & (toks < 151936))
