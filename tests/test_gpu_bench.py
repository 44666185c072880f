"""GPU: a plain `bench.py` run end to end at a small shape -- the result line's headline fields, the
number of timed steps, and --dump-outputs: the last timed step's trajectory as float arrays, the same
from run to run (seeded scenes, policy and sampling)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, T, STEPS = 64, 8, 2


def _run(outdir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                          "--warmup", "1", "--envs", str(E), "--horizon", str(T), "--dump-outputs", str(outdir)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-800:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1  # one JSON result line, nothing else on stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(outdir, f)) for f in sorted(os.listdir(outdir))}


def test_plain_run_line_and_dumped_trajectory(tmp_path):
    line, a = _run(tmp_path / "a")
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["n_gpus"] == 1
    assert line["steps"] == STEPS and line["full"] is False and "f32 policy" in line["dtype"]
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: E * T env-steps per timed step
    assert abs(line["value"] - E * T / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for leg in ("env_roofline", "env_fused", "score_pairs", "ppo_samples_per_s", "ppo_samples_per_s_mb64",
                "e2e_iteration", "dropin_loop", "cpu_baseline", "cpu_env_baseline"):
        assert line[leg] is None, leg  # --full only
    shapes = {"obs": (T + 1, E, 5, 14), "actions": (T, E), "logp": (T, E), "values": (T, E), "rewards": (T, E),
              "dones": (T, E), "info": (T, E, 8), "last_values": (1, E), "returns": (T, E), "advantages": (T, E)}
    assert {k: v.shape for k, v in a.items()} == shapes
    f64 = {"rewards", "info"}
    assert all(v.dtype == (np.float64 if k in f64 else np.float32) for k, v in a.items())
    assert all(np.isfinite(v).all() for v in a.values())
    assert set(np.unique(a["actions"])) <= {0.0, 1.0} and set(np.unique(a["dones"])) <= {0.0, 1.0}
    assert (a["logp"] <= 0).all() and a["logp"].min() < 0  # log-probabilities of sampled actions, written
    assert abs(float(a["advantages"].mean())) < 1e-3 and a["advantages"].std() > 0.5  # normalised over the batch
    line_b, b = _run(tmp_path / "b")
    assert sorted(b) == sorted(a)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
