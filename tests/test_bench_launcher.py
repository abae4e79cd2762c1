"""bench.py --gpus N must start its own N ranks (the reference's initializeProcesses ... sumAcrossProcesses,
Drivers/monteCarloDriver.f95:187, 1151-1166).  Rehearsed here on CPU: --dry-run swaps RCCL for gloo and skips
the tracing, everything else (child launcher, rendezvous on 127.0.0.1, collective, ONE JSON line from rank 0)
is the code path of the real run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "stdout must carry exactly one JSON line, got: %r" % lines
    return json.loads(lines[0])


def test_gpus_2_starts_two_ranks_and_reduces():
    out = _run("--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1")
    assert out["n_gpus"] == 2 and out["config"]["world_size"] == 2
    assert out["config"]["ranks_seen"] == [0, 1]
    assert out["config"]["photons_all_ranks_per_step"] == 2 * 10 ** 7  # the header of the reduced moment array
    assert out["steps"] == 2 and out["warmup"] == 1 and out["scaling"] == "weak"


def test_gpus_1_stays_in_process():
    out = _run("--dry-run")
    assert out["n_gpus"] == 1 and out["config"]["ranks_seen"] == [0]


def test_under_a_launcher_the_env_decides():
    """The driver's own launch line: torch.distributed.run starts the ranks, bench.py must not start more."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29631", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--dry-run", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1
    assert json.loads(lines[0])["config"]["ranks_seen"] == [0, 1]


def test_steps_must_be_at_least_one():
    """--steps is the number of timed steps that ms_per_step divides by: none is refused, not reported."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "0"], capture_output=True,
                       text=True, timeout=600)
    assert p.returncode != 0 and "--steps" in p.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900, method="thread")
def test_dump_outputs_hold_the_last_timed_step_and_repeat(tmp_path):
    """--dump-outputs DIR: the statistics of the last timed step's moments, float64, one .npy per name; the same arguments
    give the same photons, and the fixed-point tallies the same numbers bit for bit."""
    args = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-secondary"]
    outs = [_run(*args, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for out in outs:
        assert out["steps"] == 2 and out["ms_per_step"] > 0
    names = sorted(f for f in os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for k in ("totalPhotons", "batches", "meanFluxUp", "meanFluxDown", "meanFluxAbsorbed", "fluxUp", "fluxUp_StdErr",
              "absorbedVolume"):
        assert k + ".npy" in names, k
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 * 2 ** 20
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    for f in names:
        assert got[f[:-4]].dtype == np.float64, f
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f)), f
    assert got["totalPhotons"] == outs[0]["config"]["photons_in_reduced_moments_last_step"] == 10 ** 7
    assert got["fluxUp"].shape == (32, 1) and got["absorbedVolume"].shape == (32, 1, 32)
    assert abs(got["meanFluxUp"] + got["meanFluxDown"] + got["meanFluxAbsorbed"] - 1.0) < 0.03
