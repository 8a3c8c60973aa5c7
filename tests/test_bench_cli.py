"""bench.py's multi-GPU launcher on CPU: `--gpus 2` relaunches itself under torch.distributed.run
(before any GPU call) into 2 ranks, which rendezvous on 127.0.0.1, run the barrier / timed loop /
max-over-ranks skeleton, and rank 0 prints ONE JSON line with n_gpus = 2.  The stub step and the gloo
backend replace the GPU step and RCCL (the 8-GPU run is the driver's)."""
import json
import os
import subprocess
import sys

from conftest import ROOT


def test_bench_gpus2_relaunch_reports_two_ranks():
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                        "--mode", "stub", "--steps", "3", "--warmup", "1",
                        # `--n` abbreviates several of torch.distributed.run's options: the relaunch must
                        # not hand it to that parser (bench.py passes its arguments in the environment)
                        "--n", "64"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["backend"] == "gloo"


def test_bench_dump_outputs_repeatable(tmp_path):
    """`--dump-outputs DIR` writes the last step's outputs as float .npy files within 64 MB, the same from
    run to run, and `--steps` sets what they hold; `--full` is accepted (the stub has nothing behind it)."""
    import numpy as np

    def run(d, steps, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--mode", "stub",
                            "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(d), *extra],
                           cwd=ROOT, env=dict(os.environ, CUDA_VISIBLE_DEVICES=""), capture_output=True, text=True,
                           timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] >= 0
        files = sorted(os.listdir(d))
        assert files and all(f.endswith(".npy") for f in files)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
        return {f: np.load(os.path.join(d, f)) for f in files}

    a, b, c = run(tmp_path / "a", 3), run(tmp_path / "b", 3, "--full"), run(tmp_path / "c", 4)
    assert a.keys() == b.keys() == c.keys()
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], b[k])
        assert not np.array_equal(a[k], c[k])  # one more step, another state
