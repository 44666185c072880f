"""The training driver (uavhip/fit.py) on the GPU: it runs the loop a user would write by hand, it
continues after a stop bit for bit, its observers (diagnostics, evaluation) leave the training stream
alone, target_kl cuts the epochs, and it writes the files it promises.

Shape of every run: 64 envs of 4 x 4 (episodes last at most 16 steps), horizon 16, minibatch 256,
fresh scenes every 2 episodes -- so episode resets, full resets and episodes carried across iterations
all occur within the few iterations a test runs. The runs are built once per module and shared."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import dropin_env, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

SHAPE = dict(envs=64, uavs=4, targets=4, horizon=16, minibatch=256)
SEED = 5
RESET = 2
VOLATILE = ("wall_s", "env_steps_per_s")


def make_run(out, **kw):
    from uavhip.fit import TrainingRun
    args = dict(SHAPE, out_dir=str(out), seed=SEED, reset_episodes=RESET)
    args.update(kw)
    return TrainingRun(**args)


def snapshot(run):
    tr = run.trainer
    s = {k: getattr(tr, k).detach().cpu().clone() for k in ("params", "adam_m", "adam_v", "adam_step")}
    s["istate"] = run.env.istate.cpu().clone()
    s["dstate"] = run.env.dstate.cpu().clone()
    return s


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def progress(out):
    with open(os.path.join(str(out), "progress.jsonl")) as fh:
        return [json.loads(line) for line in fh]


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """Four iterations in one TrainingRun (diagnostics on, evaluation off): snapshots after 2 and 4;
    fit(2) leaves state_it2.pt behind."""
    out = tmp_path_factory.mktemp("straight")
    run = make_run(out)
    run.fit(2)
    at2 = snapshot(run)
    run.fit(4)
    return {"out": out, "at2": at2, "at4": snapshot(run), "run": run}


@pytest.fixture(scope="module")
def observed(tmp_path_factory):
    """Three iterations with every observer and every file: evaluation and diagnostics each iteration,
    checkpoint_every=1; a snapshot after 2."""
    out = tmp_path_factory.mktemp("observed")
    run = make_run(out, eval_every=1, eval_scenes=32, diagnostics_every=1, checkpoint_every=1)
    run.step()
    run.step()
    at2 = snapshot(run)
    summary = run.fit(3)
    return {"out": out, "at2": at2, "summary": summary}


def test_driver_equals_the_hand_written_loop(straight):
    """RolloutEngine + FusedPPOTrainer chained by hand with the documented seeding (eager rollout
    launches, no graph): after 2 iterations the flat parameters are the driver's, bitwise."""
    from uavhip.config import cfg
    from uavhip.policy import TransformerActorCritic
    from uavhip.rollout import RolloutEngine
    from uavhip.train import FusedPPOTrainer
    from uavhip.vec_env import VecUAVEnv
    dev = torch.device("cuda:0")
    E, N, M, T, mb = (SHAPE[k] for k in ("envs", "uavs", "targets", "horizon", "minibatch"))
    torch.manual_seed(SEED)
    policy = TransformerActorCritic().to(dev)
    env = VecUAVEnv(E, N, M, device=dev, seed=SEED, full_reset_period=RESET)
    eng = RolloutEngine(env, policy, T, seed=SEED)
    eng.start()
    trainer = FusedPPOTrainer(policy, mb)
    tr, n = eng.traj, T * E
    trainer.set_buffers(tr.obs[:T].reshape(n, 5, 14), tr.actions.reshape(n), tr.logp.reshape(n), tr.values.reshape(n),
                        tr.ret.reshape(n), tr.adv.reshape(n))
    gen = torch.Generator().manual_seed(SEED)
    for _ in range(2):
        eng.collect()
        trainer.run(epochs=cfg.K_EPOCHS, generator=gen)
    torch.cuda.synchronize()
    assert same_bits(trainer.params.cpu(), straight["at2"]["params"])
    assert same_bits(trainer.adam_step.cpu(), straight["at2"]["adam_step"])
    assert same_bits(env.istate.cpu(), straight["at2"]["istate"])
    # the shape does what the module docstring says: episodes ended, scenes were replaced
    from uavhip import _lib
    ist = straight["at4"]["istate"]
    assert int(ist[:, _lib.IST["EPISODE"]].min()) > RESET and int(ist[:, _lib.IST["SCENE_GEN"]].max()) > 1


def test_resume_is_exact(straight, tmp_path):
    """2 iterations, a new TrainingRun resumed from state_it2.pt, 2 more == 4 iterations in one run."""
    state = os.path.join(str(straight["out"]), "state_it2.pt")
    assert os.path.isfile(state)
    run = make_run(tmp_path / "resumed", resume=state)
    assert run.iteration == 2
    for k, v in snapshot(run).items():
        assert same_bits(v, straight["at2"][k]), k
    run.fit(4)
    for k, v in snapshot(run).items():
        assert same_bits(v, straight["at4"][k]), k
    a, b = progress(straight["out"]), progress(tmp_path / "resumed")
    assert [r["iteration"] for r in a] == [1, 2, 3, 4] and [r["iteration"] for r in b] == [3, 4]
    for ra, rb in zip(a[2:], b):
        assert list(ra) == list(rb)
        for k in ra:
            if k not in VOLATILE:
                assert ra[k] == rb[k], (ra["iteration"], k, ra[k], rb[k])
    # a run directory resumes from its latest state; another shape is refused by name
    import shutil
    same = tmp_path / "same"
    shutil.copytree(str(straight["out"]), str(same))
    again = make_run(same, resume=str(same))
    assert again.iteration == 4 and len(progress(same)) == 4
    # resumed in place from the older state: the lines it is about to write again are dropped
    older = make_run(same, resume=str(same / "state_it2.pt"))
    assert older.iteration == 2 and [r["iteration"] for r in progress(same)] == [1, 2]
    with pytest.raises(ValueError, match="resume: horizon differs"):
        make_run(tmp_path / "other", resume=state, horizon=32)


def test_observers_do_not_perturb(straight, observed, tmp_path):
    """Evaluation and diagnostics every iteration vs both off: bitwise equal parameters."""
    bare = make_run(tmp_path / "bare", eval_every=0, diagnostics_every=0)
    bare.fit(2)
    got = snapshot(bare)
    for k, v in got.items():
        assert same_bits(v, observed["at2"][k]), k
        assert same_bits(v, straight["at2"][k]), k
    line = progress(tmp_path / "bare")[-1]
    assert "approx_kl" not in line and "eval_mean_J" not in line
    assert "approx_kl" in progress(observed["out"])[0] and "eval_mean_J" in progress(observed["out"])[0]


def test_target_kl_zero_runs_one_epoch(tmp_path):
    """target_kl=0.0: the approximate KL after the first epoch is positive, so every iteration runs
    one epoch -- the parameters of a run with epochs=1, bitwise."""
    early = make_run(tmp_path / "early", target_kl=0.0)
    early.fit(2)
    lines = progress(tmp_path / "early")
    assert [r["epochs_run"] for r in lines] == [1, 1]
    assert all(r["approx_kl"] > 0.0 and r["optimizer_steps"] == 4 for r in lines)
    one = make_run(tmp_path / "one", epochs=1)
    one.fit(2)
    assert [r["epochs_run"] for r in progress(tmp_path / "one")] == [1, 1]
    a, b = snapshot(early), snapshot(one)
    for k in a:
        assert same_bits(a[k], b[k]), k
    assert float(a["adam_step"]) == 8.0


def test_files(observed):
    from uavhip import fit
    from uavhip.checkpoint import load_checkpoint
    from uavhip.policy import TransformerActorCritic
    from uavhip.solve import AllocationSolver
    out = str(observed["out"])
    names = set(os.listdir(out))
    want = {"checkpoint_it1.pth", "checkpoint_it2.pth", "checkpoint_it3.pth", "final_model.pth", "best_model.pth",
            "state_it2.pt", "state_it3.pt", "progress.jsonl"}
    assert want <= names and "state_it1.pt" not in names, names  # the latest two states are kept
    assert observed["summary"]["final_model"] == os.path.join(out, "final_model.pth")
    dev = torch.device("cuda:0")
    net = TransformerActorCritic().to(dev)
    rep = load_checkpoint(net, os.path.join(out, "final_model.pth"), strict=True)
    assert rep.complete and len(rep.loaded) == 50
    alloc = AllocationSolver(net, SHAPE["uavs"], SHAPE["targets"]).solve(num_scenes=8, seed=0).cpu()
    assert alloc.assignment.shape == (8, SHAPE["uavs"]) and bool(torch.isfinite(alloc.J).all())
    state = torch.load(os.path.join(out, "state_it3.pt"), map_location="cpu", weights_only=True)
    assert state["format"] == fit.STATE_FORMAT and state["run.iteration"] == 3
    for k in ("trainer.params", "trainer.adam_m", "trainer.adam_v", "trainer.adam_step", "engine.counter",
              "engine.obs_T", "env.scene.p_dmg", "env.scene.uav_pos", "env.nh_final", "env.nh_pure", "env.t_cost",
              "env.n_lock", "env.assigned", "env.istate", "env.dstate", "env.window", "stats.acc", "generator.state"):
        assert isinstance(state[k], torch.Tensor), k
    assert state["env.scene.p_dmg"].shape[0] == 2 * SHAPE["envs"]  # both scene buffers
    lines = progress(out)
    assert [r["iteration"] for r in lines] == [1, 2, 3]
    for r in lines:
        assert list(r)[:len(fit.PROGRESS_FIELDS)] == list(fit.PROGRESS_FIELDS)
        assert set(fit.DIAG_FIELDS) <= set(r) and set(fit.EVAL_FIELDS) <= set(r)
        for k, v in r.items():
            assert v is None or (isinstance(v, (int, float)) and math.isfinite(v)), (k, v)
        assert r["env_steps"] == r["iteration"] * SHAPE["envs"] * SHAPE["horizon"]
        assert r["episodes"] > 0 and r["optimizer_steps"] == 20 and r["epochs_run"] == 5
        assert 0.0 <= r["eval_beats_baseline"] <= 1.0 and r["eval_mean_J_baseline"] == lines[0]["eval_mean_J_baseline"]


def test_command_line(tmp_path):
    out = tmp_path / "cli"
    cmd = [sys.executable, "-m", "uavhip.fit", "--iterations", "2", "--envs", "64", "--uavs", "4", "--targets", "4",
           "--horizon", "16", "--minibatch", "256", "--seed", str(SEED), "--reset-episodes", str(RESET),
           "--out", str(out)]
    res = subprocess.run(cmd, env=dropin_env(), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    last = json.loads(res.stdout.strip().splitlines()[-1])
    assert last["final_model"].endswith("final_model.pth") and os.path.isfile(last["final_model"])
    assert last["iterations"] == 2 and last["env_steps"] == 2 * 64 * 16 and last["env_steps_per_s"] > 0
    assert len(progress(out)) == 2
