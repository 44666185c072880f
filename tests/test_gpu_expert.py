"""uavhip_expert_steps on the GPU (k_expert_steps): follow mode against one best-response sweep
(uavhip_refine_assignments), relabel mode against expert_np (tests/test_expert_host.py) fed the device's
pair tables and against uavhip_env_step replaying the recorded actions (bitwise), mixed mode, a
learner's decode trace, and uavhip.imitate's "expert" / "dagger" sources.

Shapes (N, M, E): 4 x 4 x 6, 5 x 7 x 33 (the last workgroup of four waves is partial), 16 x 32 x 32,
33 x 34 x 3, and two targets per lane: 3 x 70 x 5, 8 x 128 x 4; n_max = N * M."""
import functools
import math

import numpy as np
import pytest
import torch

import capi_host
from conftest import has_gpu
from test_expert_host import expert_np, flipped_traces, gpu_cases, trace_array
from test_gpu_solve import gpu_policy
from test_gpu_teacher import STATE, assert_state_equal, make_env, state_of
from test_refine_host import RTOL_J, host_scenes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

PER_STEP = ("obs", "actions", "labels", "margin", "reward", "done")  # [n_max, E, ...]
PER_ENV = ("steps", "finished", "ep_return", "stats")                # [E, ...]


_entry_point = capi_host._entry_point("uavhip_expert_steps")


@functools.lru_cache(maxsize=None)
def launch(N, M, E, omega, mode):
    """One uavhip_expert_steps launch of a case from a reset, shared by the tests (read only):
    mode "follow" (no trace), "relabel" (the flipped traces), "mixed" (the traces, the even envs
    following). -> (outputs, the env's state after, the env's window before, the env)."""
    env = make_env(host_scenes(N, M, E), N, M, omega)
    first = env.window.clone()
    trace = follow = None
    if mode != "follow":
        trace = torch.from_numpy(trace_array(flipped_traces(N, M, E, omega), N * M)).to(env.device)
    if mode == "mixed":
        follow = torch.zeros(E, dtype=torch.uint8, device=env.device)
        follow[::2] = 1
    out = env.expert_steps(trace, follow)
    torch.cuda.synchronize()
    assert not bool(env.errors().any())
    return out, state_of(env), first, env


def assert_held_rows(out):
    held = out["actions"] < 0
    assert torch.equal(held, out["labels"] < 0)
    assert bool((out["actions"][held] == -1).all()) and bool((out["labels"][held] == -1).all())
    assert not bool(out["obs"][held].any()) and not bool(out["margin"][held].any())
    assert not bool(out["reward"][held].any()) and bool((out["done"][held] == 1).all())
    live = ~held
    assert bool(((out["actions"][live] == 0) | (out["actions"][live] == 1)).all())
    assert bool(((out["labels"][live] == 0) | (out["labels"][live] == 1)).all())
    # valid rows are a prefix of every env's column, steps their number
    T = held.shape[0]
    assert torch.equal(live, torch.arange(T, device=held.device)[:, None] < out["steps"][None, :])
    return held


@pytest.mark.parametrize("N,M,E,omega", gpu_cases())
def test_follow_mode(N, M, E, omega):
    """actions_in = NULL: the labels are the actions, the env ends on the allocation of
    refine_assignments(None, max_sweeps=1) bit for bit with its J to the reward bar, rejects nothing,
    and takes sum_u (a[u] >= 0 ? a[u] + 1 : M) steps."""
    from uavhip import _lib
    out, _, first, env = launch(N, M, E, omega, "follow")
    want, J, _, _ = env.refine_assignments(None, max_sweeps=1)
    torch.cuda.synchronize()
    assert out["obs"].shape == (N * M, E, 5, 14) and out["stats"].shape == (E, 3)
    assert torch.equal(out["labels"], out["actions"]) and torch.equal(out["obs"][0], first)
    assert torch.equal(env.assigned_target_ids().to(torch.int32), want)
    Je = env.dstate[:, _lib.DST["J"]]
    err = ((Je - J).abs() / J.abs().clamp(min=1.0)).max().item()
    a = env.assigned
    steps = torch.where(a >= 0, a + 1, torch.full_like(a, M)).sum(1).to(torch.int32)
    print(f"({N}, {M}, {E}) omega {omega}: steps {int(steps.min())}..{int(steps.max())}, mean J {Je.mean().item():.6f}, "
          f"max err vs one sweep's J {err:.2e} (bar {RTOL_J:g})")
    assert err <= RTOL_J
    assert not bool(out["stats"].any()) and bool(out["finished"].all())
    assert torch.equal(out["steps"], steps)
    assert_held_rows(out)
    live = out["labels"] >= 0
    m, l = out["margin"][live], out["labels"][live]
    assert bool((m[l == 1] >= 0).all()) and bool((m[l == 0] <= 0).all())


@pytest.mark.parametrize("N,M,E,omega", gpu_cases())
def test_relabel_mode(N, M, E, omega):
    """The flipped traces: actions, labels, done, steps, finished and stats are expert_np's on the
    device's pair tables exactly, margin bit for bit (both sides do the same IEEE operations in the
    same order); windows, rewards, done flags and the final env tensors are bitwise
    uavhip_env_step(T = N * M, auto_reset = 0) replaying `actions` on a second env."""
    scenes = host_scenes(N, M, E)
    runs = flipped_traces(N, M, E, omega)
    out, state, first, env = launch(N, M, E, omega, "relabel")
    T = N * M
    trace = trace_array(runs, T)
    act, lab, mar, done = (out[k].cpu().numpy() for k in ("actions", "labels", "margin", "done"))
    steps, fin, stats = (out[k].cpu().numpy() for k in ("steps", "finished", "stats"))
    assert np.array_equal(act, trace)  # the walk is the oracle's: every trace was taken to its end
    pd, pp = env.p_dmg.cpu().numpy(), env.p_pen.cpu().numpy()
    for e, sc in enumerate(scenes):
        want = expert_np(sc, omega, trace=list(trace[:, e]), tables=(pd[e], pp[e]))
        n = want["steps"]
        assert steps[e] == n and fin[e] == want["finished"] == 1, e
        assert np.array_equal(act[:n, e], np.array(want["actions"], np.int8)), e
        assert np.array_equal(lab[:n, e], np.array(want["labels"], np.int8)), e
        assert np.array_equal(done[:n, e], np.array(want["dones"], np.uint8)), e
        assert list(stats[e]) == [want["rejected"], want["differ"], 0], e
        assert np.array_equal(mar[:n, e], np.array(want["margins"])), e
    print(f"({N}, {M}, {E}) omega {omega}: {int(steps.sum())} rows, {int((lab == 1).sum())} label-1, "
          f"{int(stats[:, 1].sum())} differ, {int(stats[:, 0].sum())} rejected")
    assert (lab == 1).any() and (lab == 0).any() and stats[:, 1].sum() > 0
    assert omega == 0.0 or stats[:, 0].sum() > 0
    held = assert_held_rows(out)
    assert bool(held.any())
    # the anchor: the recorded actions (-1 -> 0) replayed through uavhip_env_step
    twin = make_env(scenes, N, M, omega)
    o2, r2, d2, _ = twin.step(out["actions"].clamp(min=0), auto_reset=False, want_info=False)
    torch.cuda.synchronize()
    valid = ~held
    assert torch.equal(out["obs"][0], first)
    assert torch.equal(out["obs"][1:][valid[1:]], o2[:-1][valid[1:]])
    assert torch.equal(out["reward"][valid], r2[valid]) and torch.equal(out["done"][valid], d2[valid])
    assert_state_equal(state, state_of(twin, drop_error=True), "replay")
    ret, rew = np.zeros(E), out["reward"].cpu().numpy()
    for t in range(T):  # the rewards in step order (held rows add 0.0)
        ret = ret + rew[t]
    assert np.array_equal(out["ep_return"].cpu().numpy(), ret)


@pytest.mark.parametrize("N,M,E,omega", gpu_cases())
def test_mixed_mode(N, M, E, omega):
    """follow set on the even envs: every env's rows and final state are those of its own mode."""
    mixed, state, _, _ = launch(N, M, E, omega, "mixed")
    for mode, sel in (("follow", slice(0, None, 2)), ("relabel", slice(1, None, 2))):
        want, wstate, _, _ = launch(N, M, E, omega, mode)
        for k in PER_STEP:
            assert torch.equal(mixed[k][:, sel], want[k][:, sel]), (mode, k)
        for k in PER_ENV:
            assert torch.equal(mixed[k][sel], want[k][sel]), (mode, k)
        for k in STATE:
            assert torch.equal(state[k][sel], wstate[k][sel]), (mode, k)


@pytest.mark.parametrize("N,M,E", [(5, 7, 33), (16, 32, 32)])
def test_a_learners_trace(N, M, E):
    """The sampled decode of the test policy of tests/test_gpu_solve.py, traced, then walked again by
    uavhip_expert_steps: the same env (the trace's -1 rows meet finished envs: no trace ends), held
    rows with their sentinels, and a call split in two equals one call."""
    from uavhip.policy import rowproj_buffer
    omega = 0.5
    scenes = host_scenes(N, M, E)
    T = N * M
    dec = make_env(scenes, N, M, omega)
    dev = dec.device
    obs2 = torch.zeros(2, E, 5, 14, device=dev)
    dec.reset(episode=1, obs_out=obs2[0])
    steps = torch.zeros(E, dtype=torch.int32, device=dev)
    fin = torch.zeros(E, dtype=torch.uint8, device=dev)
    ret = torch.zeros(E, dtype=torch.float64, device=dev)
    trace = torch.full((T, E), 7, dtype=torch.int8, device=dev)
    gpu_policy(N, M, 1).decode_steps(dec, obs2, rowproj_buffer(E, dev), 0, True, steps, fin, actions=trace,
                                     ep_return=ret, greedy_stride=0, seed=3, offset=0, offset_stride=E)
    torch.cuda.synchronize()
    assert bool(fin.all()) and bool((trace == -1).any()) and bool((trace == 1).any()) and bool((trace == 0).any())
    one = make_env(scenes, N, M, omega)
    full = one.expert_steps(trace)
    torch.cuda.synchronize()
    for k in ("istate", "dstate", "assigned"):
        assert torch.equal(getattr(one, k), getattr(dec, k)), k
    assert torch.equal(full["actions"], trace) and torch.equal(full["steps"], steps)
    assert torch.equal(full["ep_return"], ret)
    assert not bool(full["stats"][:, 2].any()) and bool(full["finished"].all())
    assert bool(assert_held_rows(full).any())
    agree = 1.0 - float(full["stats"][:, 1].sum()) / float(steps.sum())
    print(f"({N}, {M}, {E}): {int(steps.sum())} rows, {int((full['labels'] == 1).sum())} label-1, the policy takes the "
          f"label on {agree:.3f} of them, {int(full['stats'][:, 0].sum())} rejected assigns")
    k1 = 2 * N + 1
    two = make_env(scenes, N, M, omega)
    a = two.expert_steps(trace[:k1].contiguous())
    assert not bool(a["finished"].all()) and int(a["steps"].max()) == k1
    b = two.expert_steps(trace[k1:].contiguous(), steps=a["steps"], ep_return=a["ep_return"])
    torch.cuda.synchronize()
    for k in ("obs", "actions", "labels", "margin", "reward", "done"):
        assert torch.equal(torch.cat([a[k], b[k]]), full[k]), k
    assert torch.equal(b["steps"], full["steps"]) and torch.equal(b["ep_return"], full["ep_return"])
    assert torch.equal(b["finished"], full["finished"])
    assert torch.equal(a["stats"][:, :2] + b["stats"][:, :2], full["stats"][:, :2])
    assert_state_equal(state_of(two), state_of(one), "two calls")


def test_a_trace_that_ends_holds_the_env():
    """A value outside {0, 1} on a live env: held from that step (the state of the steps before it),
    finished 0, stats[2] 1; an env that follows ignores its trace."""
    N, M, E, omega = 5, 7, 33, 0.5
    scenes = host_scenes(N, M, E)
    T, cut = N * M, N - 1
    env, short = make_env(scenes, N, M, omega), make_env(scenes, N, M, omega)
    trace = torch.from_numpy(trace_array(flipped_traces(N, M, E, omega), T)).to(env.device)
    bad = trace.clone()
    bad[cut] = torch.tensor([-1, 2, 7, -128, 127], dtype=torch.int8).repeat(E // 5 + 1)[:E].to(env.device)
    follow = torch.zeros(E, dtype=torch.uint8, device=env.device)
    follow[:4] = 1
    out = env.expert_steps(bad, follow)
    part = short.expert_steps(trace[:cut].contiguous())
    torch.cuda.synchronize()
    ref, _, _, _ = launch(N, M, E, omega, "follow")
    cutoff = ~follow.bool()
    assert torch.equal(out["stats"][:, 2], cutoff.to(torch.int32)) and torch.equal(out["finished"], follow)
    assert bool((out["steps"][cutoff] == cut).all()) and bool((out["actions"][cut:, cutoff] == -1).all())
    assert_held_rows(out)
    for k in ("obs", "actions", "labels", "margin", "reward", "done"):
        assert torch.equal(out[k][:cut, cutoff], part[k][:, cutoff]), k
        assert torch.equal(out[k][:, :4], ref[k][:, :4]), k
    got, want = state_of(env), state_of(short)
    for k in STATE:
        assert torch.equal(got[k][cutoff], want[k][cutoff]), k
    assert not bool(env.errors().any())


def test_argument_checks():
    from uavhip import _lib
    from uavhip.vec_env import VecUAVEnv
    N, M, E = 4, 4, 6
    env = make_env(host_scenes(N, M, E), N, M, 0.0)
    before = state_of(env)
    dev = env.device
    trace = torch.zeros(N * M, E, dtype=torch.int8, device=dev)
    follow = torch.ones(E, dtype=torch.uint8, device=dev)
    steps = torch.zeros(E, dtype=torch.int32, device=dev)
    fin = torch.zeros(E, dtype=torch.uint8, device=dev)
    fn, err = _lib.LIB.uavhip_expert_steps, _lib.LIB.uavhip_last_error
    p = _lib.ptr

    def call(desc, a, f, n_max, s=steps, d=fin):
        return fn(desc, p(a), p(f), n_max, None, None, None, None, None, None, p(s), p(d), None, None,
                  _lib.stream_handle())

    assert call(env.desc, trace, None, 0) == -1 and b"uavhip_expert_steps" in err() and b"n_max=0" in err()
    assert call(env.desc, None, follow, 4) == -1 and b"follow needs actions_in" in err()
    assert call(env.desc, trace, None, 4, s=None) == -1 and b"non-NULL" in err()
    assert call(env.desc, trace, None, 4, d=None) == -1 and b"non-NULL" in err()
    half = VecUAVEnv(E, N, M, 1, 1, full_reset_period=0, obs_dtype=torch.float16)
    assert call(half.desc, trace, None, 4) == -1 and b"f32 observations only" in err()
    with pytest.raises(TypeError, match="f32 observations only"):
        half.expert_steps()
    with pytest.raises(ValueError, match="n_max=0"):
        env.expert_steps(n_max=0)
    with pytest.raises(ValueError, match="follow needs actions"):
        env.expert_steps(None, follow)
    with pytest.raises(ValueError, match="actions: need a contiguous torch.int8"):
        env.expert_steps(trace.cpu())
    torch.cuda.synchronize()
    assert_state_equal(state_of(env), before, "refused calls")
    # every output but steps / finished is nullable: the all-skip trace walks N * M steps
    assert call(env.desc, trace, None, N * M) == 0
    torch.cuda.synchronize()
    assert bool((steps == N * M).all()) and bool(fin.all()) and bool((env.assigned == -1).all())


def test_imitation_sources(tmp_path):
    """source="dagger": two runs with one seed end bitwise equal; iteration 1 is source="expert"'s;
    iteration 2's rows are a hand-built decode + expert_steps from the seeding contract
    (uavhip/imitate.py's docstring)."""
    import json

    from uavhip.imitate import ImitationRun
    from uavhip.policy import rowproj_buffer
    from uavhip.vec_env import VecUAVEnv
    E, N, M, MB, seed, share = 64, 4, 4, 64, 3, 0.25
    kw = dict(envs=E, uavs=N, targets=M, minibatch=MB, seed=seed, epochs=2)
    a = ImitationRun(out_dir=str(tmp_path / "a"), source="dagger", **kw)
    x = ImitationRun(out_dir=str(tmp_path / "x"), source="expert", **kw)
    a.fit(1)
    x.fit(1)
    assert torch.equal(a.trainer.params, x.trainer.params)
    assert a.batch.follow is None and torch.equal(a.batch.actions, a.batch.taken)
    # iteration 2 by hand, with the policy as iteration 1 left it
    dev = a.device
    env = VecUAVEnv(E, N, M, device=dev, seed=seed, full_reset_period=0, scene_buffers=1)
    env.desc.seed = seed + 2
    env.istate.zero_()
    env.generate_scenes()
    obs2 = torch.zeros(2, E, 5, 14, device=dev)
    env.reset(episode=1, obs_out=obs2[0])
    steps = torch.zeros(E, dtype=torch.int32, device=dev)
    fin = torch.zeros(E, dtype=torch.uint8, device=dev)
    trace = torch.empty(N * M, E, dtype=torch.int8, device=dev)
    a.policy.packed_weights()
    a.policy.decode_steps(env, obs2, rowproj_buffer(E, dev), 0, True, steps, fin, actions=trace, greedy_stride=0,
                          seed=seed + 2, offset=0, offset_stride=E)
    follow = torch.zeros(E, dtype=torch.uint8, device=dev)
    follow[:math.ceil(share * E)] = 1
    env.reset()
    want = env.expert_steps(trace, follow)
    torch.cuda.synchronize()
    f = a.step()
    b2 = a.batch
    assert f["iteration"] == 2 and f["source"] == "dagger" and f["trace_ended"] == 0
    rows = torch.nonzero(want["labels"].reshape(-1) >= 0).reshape(-1)
    assert f["rows"] == int(rows.numel()) == int(b2.rows.numel()) and torch.equal(b2.rows.long(), rows)
    assert torch.equal(b2.obs, want["obs"]) and torch.equal(b2.actions, want["labels"])
    assert torch.equal(b2.taken, want["actions"]) and torch.equal(b2.follow, follow)
    learner = ~follow.bool()
    assert torch.equal(b2.taken[:, learner], trace[:, learner]) and bool(b2.stats[follow.bool(), 1].eq(0).all())
    differ, n = int(want["stats"][learner, 1].sum()), int(want["steps"][learner].sum())
    assert differ > 0 and abs(f["label_agreement"] - (1.0 - differ / n)) < 1e-12
    assert f["rejected_assigns"] == int(want["stats"][:, 0].sum()) == f["rejected"]
    a.fit(3)
    b = ImitationRun(out_dir=str(tmp_path / "b"), source="dagger", **kw)
    b.fit(3)
    assert torch.equal(a.trainer.params, b.trainer.params)
    assert not torch.equal(a.trainer.params, x.trainer.params)
    lines = [json.loads(s) for s in open(tmp_path / "b" / "progress.jsonl")]
    assert [s["iteration"] for s in lines] == [1, 2, 3]
    for s in lines:
        assert list(s)[:7] == ["iteration", "rows", "nll_before", "nll_after", "agreement", "teacher_mean_J", "rejected"]
        assert {"label_agreement", "assign_agreement", "rejected_assigns"} <= set(s)
    assert lines[0]["label_agreement"] is None and 0.0 < lines[1]["label_agreement"] < 1.0
    assert lines[1]["rows"] == f["rows"] and lines[1]["label_agreement"] == f["label_agreement"]
