"""uavhip_refine_assignments on the GPU (k_refine): the kernel against refine_np, the numpy restatement
of the best-response rule (tests/test_refine_host.py), fed the pair tables read back from the device
-- assignments, stats and covered exactly, J to the project's reward bar -- and the layers above it:
VecUAVEnv.refine_assignments, AllocationSolver.solve(refine=...) / baseline and the command line.

Shapes (N, M, E): the register-column path at its three capacities (4 x 4 and 5 x 7: 8; 16 x 32: 16),
the streamed path (33 x 34: N > 32) and two targets per lane (3 x 70, through VecUAVEnv alone: the
decode kernel stops at M <= 64); E = 6, 33, 3 and 5 leave the last workgroup of four waves partial."""
import copy
import itertools
import json

import numpy as np
import pytest
import torch

from test_gpu_solve import gpu_policy
from test_refine_host import (OMEGAS, RTOL_J, SHAPES, check_case_conditions, host_scenes, prm, random_starts,
                              refine_rows)

pytestmark = pytest.mark.gpu

K_DECODE = 3


def make_env(scenes, N, M, omega, scene_buffers=1):
    from uavhip.vec_env import VecUAVEnv
    v = VecUAVEnv(len(scenes), N, M, 1, 1, full_reset_period=0, scene_buffers=scene_buffers)
    v.set_params(prm(omega))
    v.load_scenes(list(scenes))
    return v


def decoded_env(scenes, N, M, omega, K):
    """An env of K replicas per scene (scene-major) with every episode finished: decoded by the test
    policy of tests/test_gpu_solve.py (replica 0 greedy, the others sampled), or, beyond the decode
    kernel's M <= 64, stepped through random actions."""
    from uavhip.policy import rowproj_buffer
    env = make_env(tuple(s for s in scenes for _ in range(K)), N, M, omega)
    E, dev = env.E, env.device
    if M <= 64:
        obs2 = torch.zeros(2, E, 5, 14, device=dev)
        env.reset(episode=1, obs_out=obs2[0])
        steps = torch.zeros(E, dtype=torch.int32, device=dev)
        fin = torch.zeros(E, dtype=torch.uint8, device=dev)
        gpu_policy(N, M, 1).decode_steps(env, obs2, rowproj_buffer(E, dev), 0, True, steps, fin, n_max=N * M,
                                         greedy_stride=K, seed=3, offset=0, offset_stride=E)
    else:
        env.reset(episode=1)
        g = torch.Generator().manual_seed(5)
        act = (torch.rand(N * M, E, generator=g) < 0.5).to(torch.int8).to(dev)
        env.step(act, auto_reset=False, want_info=False)
    torch.cuda.synchronize()
    assert bool((env.istate[:, 0] >= N).all()), "an episode did not finish"
    return env


def tables(env, stride=1, rows=None):
    """The active scene's (p_dmg, p_pen, value, cost, tgt_id) of envs 0, stride, 2 stride, ... as numpy."""
    sel = slice(0, None if rows is None else rows * stride, stride)
    return tuple(getattr(env, k)[sel].cpu().numpy() for k in ("p_dmg", "p_pen", "tgt_value", "uav_cost", "tgt_id"))


def run_and_compare(label, env, omega, start, stride=1, rows=None, max_sweeps=32, **kw):
    """One launch against refine_np on the device's tables. Returns the restatement's rows."""
    got = env.refine_assignments(None if start is None else torch.from_numpy(start).to(env.device), stride=stride,
                                 rows=rows, max_sweeps=max_sweeps, **kw)
    torch.cuda.synchronize()
    asg, J, cov, st = (t.cpu().numpy() for t in got)
    want = refine_rows(*tables(env, stride, rows), omega, start, max_sweeps)
    err = np.abs(J - want[1]) / np.maximum(1.0, np.abs(want[1]))
    print(f"{label}: {len(J)} rows, sweeps {want[3][:, 0].min()}..{want[3][:, 0].max()}, moves {int(want[3][:, 1].sum())}, "
          f"mean J {want[1].mean():.6f}, max J err {err.max():.2e} (bar {RTOL_J:g})")
    assert asg.dtype == np.int32 and np.array_equal(asg, want[0]), label
    assert np.array_equal(st, want[3]), label
    assert np.array_equal(cov, want[2]), label
    assert bool((err <= RTOL_J).all()), (label, float(err.max()))
    return want


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("N,M,E", SHAPES)
def test_kernel_is_the_restatement(N, M, E, omega):
    scenes = host_scenes(N, M, E)
    env = make_env(scenes, N, M, omega)
    tag = f"({N}, {M}, {E}) omega {omega}"
    runs = [run_and_compare(tag + " from empty", env, omega, None),
            run_and_compare(tag + " from random ids", env, omega, random_starts(N, M, E))]
    dec = decoded_env(scenes, N, M, omega, K_DECODE)
    best, _, _, asg = dec.select_best(K_DECODE)
    assert bool((best >= 0).all())
    start = asg.cpu().numpy()
    assert (start >= 0).any()
    runs.append(run_and_compare(tag + " from best-of-3", dec, omega, start, stride=K_DECODE, rows=E))
    to_none = check_case_conditions(tag, runs)
    assert omega == 0.0 or to_none > 0


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("N,M,E", [(5, 7, 33), (16, 32, 32), (3, 70, 5)])
def test_zero_sweeps_scores_a_decode(N, M, E, omega):
    """max_sweeps = 0 on a finished env's own allocation: the env's J and covered, nothing moved."""
    from uavhip import _lib
    env = decoded_env(host_scenes(N, M, E), N, M, omega, 1)
    ids = env.assigned_target_ids().to(torch.int32).contiguous()
    asg, J, cov, st = env.refine_assignments(ids, max_sweeps=0)
    torch.cuda.synchronize()
    Je = env.dstate[:, _lib.DST["J"]]
    err = ((J - Je).abs() / Je.abs().clamp(min=1.0)).max().item()
    print(f"({N}, {M}, {E}) omega {omega}: mean J {Je.mean().item():.6f}, max err vs dstate[J] {err:.2e}")
    assert bool((ids >= 0).any()) and torch.equal(asg, ids)
    assert err <= RTOL_J
    assert torch.equal(cov, env.istate[:, _lib.IST["N_COVERED"]])
    assert torch.equal(st, torch.tensor([0, 0, 1, 0], dtype=torch.int32, device=st.device).expand(E, 4))


def test_sweep_cap():
    """max_sweeps = 1, 2, 3 from the empty assignment: the restatement cut at the same sweep, and
    'converged' only where the last sweep run made no move."""
    N, M, E, omega = 16, 32, 32, 0.5
    env = make_env(host_scenes(N, M, E), N, M, omega)
    full = refine_rows(*tables(env), omega, None, 32)
    need = full[3][:, 0]  # sweeps to convergence, the last one without a move
    assert need.min() <= 3 < need.max(), need
    for cap in (1, 2, 3):
        want = run_and_compare(f"cap {cap}", env, omega, None, max_sweeps=cap)
        assert np.array_equal(want[3][:, 2], (need <= cap).astype(np.int32))
        assert np.array_equal(want[3][:, 0], np.minimum(need, cap))
    assert bool((want[3][:, 2] == 0).any()) and bool((want[3][:, 2] == 1).any())


def test_invalid_and_duplicated_ids_and_in_place():
    N, M, E, omega = 5, 7, 33, 0.5
    scenes = [dict(s) for s in host_scenes(N, M, E)]
    for s in scenes[::2]:  # a duplicated id: the lowest list index is meant, and the id it replaced is gone
        ids = s["tgt_id"].copy()
        ids[M - 1] = ids[0]
        s["tgt_id"] = ids
    env = make_env(scenes, N, M, omega)
    start = random_starts(N, M, E)
    bad = np.random.default_rng(2).random((E, N))
    start[bad < 0.1] = M + 5
    start[(bad >= 0.1) & (bad < 0.2)] = -3
    start[0, 0], start[1, 1] = 2 ** 31 - 1, -2 ** 31
    for sweeps in (0, 32):
        want = run_and_compare(f"invalid ids, {sweeps} sweeps", env, omega, start, max_sweeps=sweeps)
        # more than the ids made invalid above: the ids the duplicates replaced match nothing either
        assert want[3][:, 3].sum() > (bad < 0.2).sum()
    buf = torch.from_numpy(start).to(env.device)
    a, J, cov, st = env.refine_assignments(buf.clone())
    b, J2, cov2, st2 = env.refine_assignments(buf, out=buf)
    torch.cuda.synchronize()
    assert b.data_ptr() == buf.data_ptr()
    for x, y in ((a, b), (J, J2), (cov, cov2), (st, st2)):
        assert torch.equal(x, y)


def test_env_is_only_read():
    N, M, E, omega = 5, 7, 33, 0.5
    env = decoded_env(host_scenes(N, M, E), N, M, omega, 1)
    names = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")
    before = {k: getattr(env, k).clone() for k in names}
    before.update({"scene/" + k: t.clone() for k, t in env._scene.items()})
    for start in (None, env.assigned_target_ids().to(torch.int32).contiguous()):
        for sweeps in (0, 32):
            env.refine_assignments(start, max_sweeps=sweeps)
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(env, k), before[k]), k
    for k, t in env._scene.items():
        assert torch.equal(t, before["scene/" + k]), k


def test_double_buffered_env_uses_the_active_scene():
    from uavhip import _lib
    N, M, E, omega = 5, 7, 9, 0.5
    a_scenes, b_scenes = host_scenes(N, M, E), host_scenes(N, M, E, 11)
    env = make_env(a_scenes, N, M, omega, scene_buffers=2)  # buffer 0, scored, SCENE_SEL = 0
    for e, s in enumerate(b_scenes):                        # buffer 1: other scenes
        for k, dst in env._scene.items():
            if k not in ("p_dmg", "p_pen", "uav_type"):
                dst[E + e].copy_(torch.as_tensor(np.asarray(s[k]).reshape(tuple(dst[E + e].shape))).to(dst.dtype))
    odd = torch.zeros(E, dtype=torch.uint8, device=env.device)
    odd[1::2] = 1
    env.istate[1::2, _lib.IST["SCENE_SEL"]] = 1
    env.score_pairs(odd)
    torch.cuda.synchronize()
    assert bool((env._scene["p_dmg"][E + 1] != env._scene["p_dmg"][1]).any())
    want = run_and_compare("scene_buffers = 2", env, omega, None)
    stale = refine_rows(*(env._scene[k][:E].cpu().numpy() for k in ("p_dmg", "p_pen", "tgt_value", "uav_cost", "tgt_id")),
                        omega, None)
    assert bool((want[1][1::2] != stale[1][1::2]).all()) and np.array_equal(want[1][::2], stale[1][::2])


def _fields(r):
    return (r.assignment, r.J, r.covered, r.best_replica, r.steps, r.replica_J)


@pytest.mark.parametrize("N,M,S,K,omega", [(5, 7, 9, 4, 0.5), (16, 32, 8, 3, 0.0)])
def test_solver_refine(N, M, S, K, omega):
    from uavhip import AllocationSolver
    from uavhip.config import Config
    cfg = Config()
    cfg.COST_WEIGHT_OMEGA = omega
    net = gpu_policy(N, M, 1)
    solver = AllocationSolver(net, N, M, samples=K, config=cfg)
    plain = solver.solve(num_scenes=S, seed=5)
    r0 = solver.solve(num_scenes=S, seed=5, refine=0)
    for x, y in zip(_fields(plain), _fields(r0)):
        assert torch.equal(x, y)
    assert r0.decoded_J is None and r0.refine_stats is None and r0.actions is None
    assert bool((r0.best_replica >= 0).all())
    r8 = solver.solve(num_scenes=S, seed=5, refine=8)
    alone = solver.env.refine_assignments(r0.assignment, stride=K, rows=S, max_sweeps=8)
    torch.cuda.synchronize()
    for x, y in zip((r8.assignment, r8.J, r8.covered, r8.refine_stats), alone):
        assert torch.equal(x, y)
    assert torch.equal(r8.decoded_J, r0.J)
    for x, y in zip(_fields(r8)[3:], _fields(r0)[3:]):
        assert torch.equal(x, y)
    gain = (r8.J - r8.decoded_J).cpu().numpy()
    print(f"({N}, {M}) K = {K} omega {omega}, untrained test policy: mean J decoded {r0.J.mean().item():.4f} -> "
          f"refined {r8.J.mean().item():.4f}, smallest change {gain.min():.2e}, moves {int(r8.refine_stats[:, 1].sum())}")
    assert bool((r8.J >= r8.decoded_J - RTOL_J * r8.J.abs()).all())
    assert int(r8.refine_stats[:, 1].sum()) > 0, "degenerate case: the refinement moved nothing"
    c = r8.cpu()
    assert c.decoded_J.device.type == "cpu" and c.refine_stats.shape == (S, 4)
    # the restatement on the solver's own scenes
    want = refine_rows(*tables(solver.env, K, S), omega, r0.assignment.cpu().numpy(), 8)
    assert np.array_equal(c.assignment.numpy(), want[0]) and np.array_equal(c.refine_stats.numpy(), want[3])


def test_solver_refines_unfinished_scenes_from_empty_and_baseline():
    from uavhip import AllocationSolver
    N, M, S, K = 5, 7, 9, 2
    net = gpu_policy(N, M, 1)
    solver = AllocationSolver(net, N, M, samples=K)
    solver.solve(num_scenes=S, seed=4)
    alone = solver.env.refine_assignments(None, stride=K, rows=S)
    torch.cuda.synchronize()
    alone = [t.clone() for t in alone]
    base = AllocationSolver(net, N, M, samples=K).baseline(num_scenes=S, seed=4)
    for x, y in zip((base.assignment, base.J, base.covered, base.refine_stats), alone):
        assert torch.equal(x, y)
    assert base.decoded_J is None and base.actions is None
    assert not bool(base.best_replica.any()) and not bool(base.steps.any()) and not bool(base.replica_J.any())
    assert base.replica_J.shape == (S, K) and bool((base.refine_stats[:, 2] == 1).all())
    assert not torch.equal(base.J, AllocationSolver(net, N, M, samples=K).baseline(num_scenes=S, seed=5).J)
    # no replica finished (the decode cut before any episode can end): refined from the empty assignment
    scenes = list(host_scenes(N, M, 4))
    cut = solver.solve(scenes=scenes, max_steps=N - 1, refine=32)
    hb = solver.baseline(scenes=scenes)
    assert bool((cut.best_replica == -1).all()) and bool((cut.decoded_J == 0).all())
    for x, y in zip((cut.assignment, cut.J, cut.covered, cut.refine_stats),
                    (hb.assignment, hb.J, hb.covered, hb.refine_stats)):
        assert torch.equal(x, y)
    assert bool((hb.assignment >= 0).any())


def test_command_line_keys(tmp_path, capsys):
    from uavhip import solve
    N, M = 5, 7
    ck = tmp_path / "policy.pth"
    torch.save(copy.deepcopy(gpu_policy(N, M, 1)).cpu().state_dict(), ck)
    argv = ["--checkpoint", str(ck), "--scenes", "8", "--samples", "2", "--uavs", str(N), "--targets", str(M)]
    today = ["scenes", "samples", "N", "M", "seed", "mean_J", "best_J", "mean_covered", "mean_steps", "unfinished",
             "scenes_per_s"]
    solve.main(argv)
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert list(plain) == today
    solve.main(argv + ["--refine", "4", "--baseline"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert list(out)[:len(today)] == today
    assert {"mean_J_decoded", "mean_J_refined", "mean_J_baseline", "policy_beats_baseline"} <= set(out)
    assert out["mean_J_decoded"] == plain["mean_J"] and out["mean_J_refined"] == out["mean_J"]
    assert out["mean_J_refined"] >= out["mean_J_decoded"] - RTOL_J * abs(out["mean_J_refined"])
    assert 0.0 <= out["policy_beats_baseline"] <= 1.0
