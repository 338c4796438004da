"""bench.py's plain run, as every measurement launches it (`bench.py --gpus 1 --steps K --warmup W`), in a fresh child
process: one timed region of exactly K steps, the headline fields and nothing of --full's records; --dump-outputs writes
what the timed rollout computed in its last step, which must be the CPU oracle's observations after W + K steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.timeout(600)
def test_plain_run_times_k_steps_and_dumps_the_oracles_observations(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import oracle
    N, W, K, WARM = 16384, 24, 64, 8
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(K), "--warmup", str(WARM),
                        "--envs", str(N), "--settle-steps", "0", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["metric"] == "env-steps/sec" and rec["unit"] == "env-steps/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "i8" and rec["steps"] == K and rec["warmup"] == WARM and rec["repeats"] == 1
    assert abs(rec["value"] - N * K / (rec["ms_per_step"] * 1e-3 * K)) <= 1e-6 * rec["value"]
    for k in ("cold_start", "per_step_launches", "resident_rollout", "temper", "dqn", "dqn_config3", "cpu_baseline"):
        assert k not in rec, k
    obs = np.load(out / "obs.npy")
    envs = np.load(out / "obs_envs.npy")
    sums = np.load(out / "obs_env_sums.npy")
    assert obs.dtype == np.float32 and envs.dtype == np.float64 and sums.dtype == np.float64
    assert 0 < len(envs) < N and obs.shape == (len(envs), 2, W + 2, W + 2) and sums.shape == (N, 2)
    ref = oracle.VecOracle(N, W, seed=0x5EED, stream=0)
    ref.reset_all()
    for _ in range(WARM + K):
        o, _, _, _ = ref.step(autoreset=True)
    idx = envs.astype(np.int64)
    assert np.array_equal(obs.reshape(len(idx), 2, -1), o[idx].astype(np.float32))
    assert np.array_equal(sums, o.astype(np.float64).sum(-1))
