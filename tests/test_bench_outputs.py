"""bench.py's plain run and --dump-outputs: a plain run prints the contract line only (the roofline, GEMM rows, decode / CPU legs and the
parity gate are --full), and the logits of the last timed step land in DIR/logits.npy, the same on every run with the same arguments."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(argv, timeout):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=timeout,
                          env=env, cwd=ROOT)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--workload", "mt-decode", "--dump-outputs", "unused"]])
def test_bench_rejects_arguments_it_cannot_honour_cpu(argv):
    """--steps sets the number of timed steps (at least one); --dump-outputs is implemented for the prefill workload: both are checked
    before any device is touched"""
    r = _run_bench(["--gpus", "1", "--warmup", "0"] + argv, 120)
    assert r.returncode == 2 and "error:" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_same_logits_on_every_run(tmp_path):
    import numpy as np
    got = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        r = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--layers", "2", "--seq", "256", "--dump-outputs", str(out)], 600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and "# bench detail" not in r.stdout, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "tokens/s" and d["config"]["valid"] is False
        assert not {"roofline", "mt_decode", "cpu_baseline", "parity"} & set(d)
        a = np.load(out / "logits.npy")
        assert a.dtype == np.float32 and a.shape == (1, 1, 32000) and np.isfinite(a).all() and np.abs(a).max() > 0
        got.append(a)
    assert np.array_equal(got[0], got[1])
