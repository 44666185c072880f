"""bench.py's evidence plumbing on the CPU (no GPU): the PMC summary lookup matches rocprofv3's
template-instance kernel names (roofline.traffic was null because k_rollout_steps<1> did
not match), the env step's traffic is dropped when it implies more than the HBM peak at the measured
time, and the weight-stream view prices one weight read per workgroup and step."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "target-allocation-ppo-transformer_amd"))


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    import bench as b
    return b


def test_kernel_base_strips_namespaces_and_templates(bench):
    assert bench._kernel_base("uavhip::pol::k_rollout_steps<1>") == "k_rollout_steps"
    assert bench._kernel_base("k_policy_forward<false, true, true>") == "k_policy_forward"
    assert bench._kernel_base("uavhip::k_gae") == "k_gae"


def test_profiled_traffic_matches_template_instances(bench, tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "r99_pmc.json").write_text(json.dumps({"pmc": {
        "uavhip::pol::k_rollout_steps<1>": {"hbm_bytes_per_launch": 123.0},
        "uavhip::k_env_step<1, false>": {"hbm_bytes_per_launch": 7.0}}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.profiled_traffic("k_rollout_steps") == (123.0, "r99_pmc.json")
    assert bench.profiled_traffic("k_env_step<1, false>") == (7.0, "r99_pmc.json")  # the exact name first
    assert bench.profiled_traffic("k_missing") == (None, None)


def test_profiled_traffic_refuses_ambiguous_template_matches(bench, tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "r99_pmc.json").write_text(json.dumps({"pmc": {
        "uavhip::pol::k_rollout_steps<1>": {"hbm_bytes_per_launch": 1.0},
        "uavhip::pol::k_rollout_steps<2>": {"hbm_bytes_per_launch": 2.0}}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.profiled_traffic("k_rollout_steps") == (None, None)


def test_env_share_reads_the_newest_summary(bench, tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "r98_env_share.json").write_text(json.dumps({"env_bytes_per_step": 1.0, "env_ns_per_step": 10.0}))
    (prof / "r99_env_share.json").write_text(json.dumps({"env_bytes_per_step": 2.0, "env_ns_per_step": 20.0}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.env_share_traffic() == (2.0, "r99_env_share.json", 20.0)


def test_weight_stream_prices_one_weight_read_per_workgroup_step(bench):
    from uavhip._lib import LIB
    n = int(LIB.uavhip_policy_layout(None, 0))
    w = bench.weight_stream(0.05, 4096)
    assert w["workgroups"] == 256 and w["bytes_per_workgroup_step"] == 4 * n
    assert abs(w["achieved"] - 4 * n * 256 / 50e-6 / 1e9) < 1e-6
    assert abs(w["frac"] - w["achieved"] / bench.L2_PEAK_GBS) < 1e-12


LEGS = ("no_ppo", "no_env_fused", "no_cpu_baseline", "no_e2e", "no_env_diff", "no_dropin")


def test_plain_run_switches_every_other_leg_off(bench):
    """Without --full only the timed rollout runs, whatever the --no-* options say; --full runs every
    leg the --no-* options do not skip."""
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 3)
    assert all(getattr(a, leg) for leg in LEGS)
    a = bench.parse(["--full"])
    assert a.full and not any(getattr(a, leg) for leg in LEGS)
    a = bench.parse(["--full", "--no-dropin", "--dump-outputs", "out"])
    assert a.no_dropin and not a.no_ppo and a.dump_outputs == "out"


def test_dump_outputs_writes_float_arrays_within_the_budget(bench, tmp_path):
    """dump_outputs: float64 stays float64, everything else becomes float32 (exactly, for the int8 /
    uint8 buffers); an array over its share of the budget keeps the same seeded envs in every call."""
    import numpy as np
    import torch
    T, E = 4, 50
    g = torch.Generator().manual_seed(0)
    outs = {"obs": torch.randn(T + 1, E, 5, 14, generator=g),
            "actions": torch.randint(0, 2, (T, E), generator=g, dtype=torch.int8),
            "dones": torch.randint(0, 2, (T, E), generator=g, dtype=torch.uint8),
            "rewards": torch.randn(T, E, generator=g, dtype=torch.float64),
            "last_values": torch.randn(1, E, generator=g)}
    budget = 5 * 4 * (T + 1) * 70 * 10  # each of the 5 arrays gets room for 10 envs of obs
    w1 = bench.dump_outputs(str(tmp_path / "a"), outs, budget=budget)
    w2 = bench.dump_outputs(str(tmp_path / "b"), outs, budget=budget)
    assert w1 == w2 and sorted(w1) == sorted(outs)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in outs}
    assert sum(a.nbytes for a in got.values()) <= budget
    assert got["rewards"].dtype == np.float64 and all(a.dtype == np.float32 for k, a in got.items() if k != "rewards")
    for k in ("actions", "dones", "rewards", "last_values"):  # within their share: whole, exact
        np.testing.assert_array_equal(got[k], outs[k].numpy().astype(got[k].dtype))
    keep = np.sort(np.random.default_rng(bench.DUMP_SEED).permutation(E)[:10])
    assert got["obs"].shape == (T + 1, 10, 5, 14)
    np.testing.assert_array_equal(got["obs"], outs["obs"].numpy()[:, keep])
    np.testing.assert_array_equal(got["obs"], np.load(tmp_path / "b" / "obs.npy"))


def test_trajectory_outputs_are_what_collect_returns(bench):
    import torch
    from types import SimpleNamespace
    T, E = 3, 8
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    tr = SimpleNamespace(obs=z(T + 1, E, 5, 14), actions=z(T, E), logp=z(T, E), values=z(T, E), rewards=z(T, E),
                         dones=z(T, E), info=z(T, E, 8), last_values=z(E), ret=z(T, E), adv=z(T, E))
    outs = bench.trajectory_outputs(tr)
    assert sorted(outs) == ["actions", "advantages", "dones", "info", "last_values", "logp", "obs", "returns",
                            "rewards", "values"]
    assert outs["obs"] is tr.obs and outs["returns"] is tr.ret and outs["last_values"].shape == (1, E)
    tr.info = None
    assert "info" not in bench.trajectory_outputs(tr)


def test_env_traffic_dropped_when_it_exceeds_the_hbm_peak(bench):
    # round 3's line: 70.9 MB per step against a 2.56 us time = 27.7 TB/s -> dropped, with the reason
    t, gbs, ok, why = bench.check_traffic(70.9e6, 2.56e-3)
    assert t is None and ok is False and gbs > bench.HBM_PEAK_GBS and "HBM peak" in why
    t, gbs, ok, why = bench.check_traffic(9.4e6, 3.0e-3)  # round 4: 9.4 MB over 3.0 us = 3.1 TB/s
    assert t == 9.4e6 and ok is True and why is None and abs(gbs - 3133.3) < 1
    assert bench.check_traffic(None, 1.0) == (None, None, None, None)
