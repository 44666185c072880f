"""uavhip_teacher_steps on the GPU (k_teacher_steps): the recorded trace replayed through
uavhip_env_step (bitwise), the omega = 0 closed forms, rejected assigns against the oracle env driven by
the same rule (tests/test_teacher_host.py teacher_np), and the conventions of the entry point: invalid
and duplicated ids, held envs, continuation calls, held rows, argument checks.

E = 64 at every shape (N, M): 4 x 4, 5 x 7, 16 x 32 (one target per lane), 33 x 34 (N > 32), 3 x 70 and
8 x 128 (two targets per lane); 16 workgroups of four waves."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from test_refine_host import RTOL_J, host_scenes, prm, random_starts
from test_teacher_host import (E, OMEGA_REJECT, SHAPES, TEACHER_SEED, closed_form_steps, teach_indices, teacher_np)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

STATE = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")


def make_env(scenes, N, M, omega):
    from uavhip.vec_env import VecUAVEnv
    v = VecUAVEnv(len(scenes), N, M, 1, 1, full_reset_period=0, scene_buffers=1)
    v.set_params(prm(omega))
    v.load_scenes(list(scenes))
    v.reset(episode=1)
    return v


def state_of(env, drop_error=False):
    from uavhip import _lib
    s = {k: getattr(env, k).clone() for k in STATE}
    if drop_error:
        s["istate"][:, _lib.IST["ERROR"]] = 0
    return s


def assert_state_equal(a, b, label):
    for k in STATE:
        assert torch.equal(a[k], b[k]), (label, k)


def dev_i32(a, env):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(env.device)


def teachers(env, N, M):
    """(label, [E, N] int32 device target ids): refine's baseline, and a random assignment."""
    base = env.refine_assignments(None)[0].clone()
    return (("baseline", base), ("random", dev_i32(random_starts(N, M, E, TEACHER_SEED), env)))


@pytest.mark.parametrize("N,M", SHAPES)
def test_replay_equality(N, M):
    """The recorded actions (-1 -> 0) replayed on a second env from the same reset through
    uavhip_env_step(T = N * M, auto_reset = 0): on every valid row obs[t + 1], reward, done and info are
    bitwise the replay's, the final env tensors too (the replay steps finished envs on and flags
    istate[ERROR]; the teacher kernel holds them). Held rows: zero window, action -1, reward 0, done 1."""
    from uavhip import _lib
    omega = 0.5
    scenes = host_scenes(N, M, E)
    T = N * M
    for label, asg in teachers(make_env(scenes, N, M, omega), N, M):
        env, twin = make_env(scenes, N, M, omega), make_env(scenes, N, M, omega)
        first = env.window.clone()
        out = env.teacher_steps(asg, want_info=True)
        obs, act, rew, done, info = (out[k] for k in ("obs", "actions", "reward", "done", "info"))
        assert obs.shape == (T, E, 5, 14) and act.shape == (T, E)
        valid = act >= 0
        steps = out["steps"]
        assert bool(out["finished"].all()) and bool((steps >= N).all()) and bool((steps <= T).all())
        assert torch.equal(valid.sum(0).to(torch.int32), steps)
        # valid rows are a prefix of every env's column
        assert torch.equal(valid, torch.arange(T, device=env.device)[:, None] < steps[None, :])
        o2, r2, d2, i2 = twin.step(act.clamp(min=0), auto_reset=False, want_info=True)
        torch.cuda.synchronize()
        print(f"({N}, {M}) {label}: steps {int(steps.min())}..{int(steps.max())}, {int(valid.sum())} valid rows, "
              f"{int((act == 1).sum())} assigns, {int(out['stats'][:, 0].sum())} rejected")
        assert torch.equal(obs[0], first)
        assert torch.equal(obs[1:][valid[:-1]], o2[:-1][valid[:-1]])
        assert torch.equal(rew[valid], r2[valid]) and torch.equal(done[valid], d2[valid])
        assert torch.equal(info[valid], i2[valid])
        assert torch.equal(done[valid].sum(), torch.tensor(E, device=env.device))  # one finishing step per env
        assert_state_equal(state_of(env), state_of(twin, drop_error=True), label)
        assert not bool(env.errors().any())
        ret, rew_host = np.zeros(E), rew.cpu().numpy()
        for t in range(T):  # the rewards in step order (held rows add 0.0)
            ret = ret + rew_host[t]
        assert np.array_equal(out["ep_return"].cpu().numpy(), ret)
        held = ~valid
        assert bool(held.any())
        assert not bool(obs[held].any()) and not bool(rew[held].any()) and bool((done[held] == 1).all())
        assert not bool(info[held].any()) and bool((act[held] == -1).all())
        assert bool(((act[valid] == 0) | (act[valid] == 1)).all())
        assert torch.equal(env.dstate[:, _lib.DST["J"]], twin.dstate[:, _lib.DST["J"]])


@pytest.mark.parametrize("N,M", SHAPES)
def test_omega_zero_closed_forms(N, M):
    from uavhip import _lib
    scenes = host_scenes(N, M, E)
    env = make_env(scenes, N, M, 0.0)
    start = random_starts(N, M, E, TEACHER_SEED)
    asg = dev_i32(start, env)
    out = env.teacher_steps(asg)
    _, Jr, _, _ = env.refine_assignments(asg, max_sweeps=0)
    torch.cuda.synchronize()
    teach = np.array([teach_indices(sc["tgt_id"], a)[0] for sc, a in zip(scenes, start)], np.int32)
    want_steps = np.array([closed_form_steps(t, M) for t in teach], np.int32)
    assert np.array_equal(env.assigned.cpu().numpy(), teach)
    assert np.array_equal(out["steps"].cpu().numpy(), want_steps)
    assert torch.equal(env.assigned_target_ids().to(torch.int32), asg)
    Je = env.dstate[:, _lib.DST["J"]]
    err = ((Je - Jr).abs() / Jr.abs().clamp(min=1.0)).max().item()
    print(f"({N}, {M}): steps {want_steps.min()}..{want_steps.max()}, mean J {Je.mean().item():.6f}, "
          f"max err vs refine's J {err:.2e} (bar {RTOL_J:g})")
    assert err <= RTOL_J
    assert not bool(out["stats"].any()) and bool(out["finished"].all())


@pytest.mark.parametrize("N,M", SHAPES)
def test_rejections_match_the_oracle(N, M):
    """omega = 2, random teacher: actions, pointers and the rejected count exactly, rewards to the
    project's reward bar, against the oracle env driven by the same rule."""
    from uavhip import _lib
    scenes = host_scenes(N, M, E)
    start = random_starts(N, M, E, TEACHER_SEED)
    env = make_env(scenes, N, M, OMEGA_REJECT)
    out = env.teacher_steps(dev_i32(start, env), want_info=True)
    torch.cuda.synchronize()
    act, rew, info = out["actions"].cpu().numpy(), out["reward"].cpu().numpy(), out["info"].cpu().numpy()
    steps, stats = out["steps"].cpu().numpy(), out["stats"].cpu().numpy()
    ids = env.assigned_target_ids().cpu().numpy()
    worst = 0.0
    for e, (sc, a) in enumerate(zip(scenes, start)):
        want = teacher_np(sc, a, OMEGA_REJECT)
        n = want["steps"]
        assert steps[e] == n, e
        assert np.array_equal(act[:n, e], np.array(want["actions"], np.int8)), e
        assert bool((act[n:, e] == -1).all()), e
        # the pointer AFTER step t is the pointer step t + 1 was decided on
        after = np.stack([info[:n, e, _lib.INFO["UAV_IDX"]], info[:n, e, _lib.INFO["TARGET_IDX"]]], 1).astype(int)
        assert np.array_equal(after[:-1], np.array(want["pointers"][1:], int)), e
        assert stats[e, 0] == want["rejected"] and stats[e, 1] == 0, e
        assert np.array_equal(ids[e], want["assigned"]), e
        r = np.array(want["rewards"])
        worst = max(worst, float((np.abs(rew[:n, e] - r) / np.maximum(1.0, np.abs(r))).max()))
    print(f"({N}, {M}) omega {OMEGA_REJECT}: {int(stats[:, 0].sum())} rejected of {int((start >= 0).sum())} teacher "
          f"assigns, max reward err {worst:.2e} (bar {RTOL_J:g})")
    assert stats[:, 0].sum() > 0
    assert worst <= RTOL_J


def test_invalid_and_duplicated_ids():
    N, M, omega = 5, 7, 0.5
    scenes = [dict(s) for s in host_scenes(N, M, E)]
    for s in scenes[::2]:  # a duplicated id: the lowest list index is meant, and the id it replaced is gone
        ids = s["tgt_id"].copy()
        ids[M - 1] = ids[0]
        s["tgt_id"] = ids
    start = random_starts(N, M, E, TEACHER_SEED)
    bad = np.random.default_rng(2).random((E, N))
    start[bad < 0.1] = M + 5
    start[(bad >= 0.1) & (bad < 0.2)] = -3
    start[0, 0], start[1, 1] = 2 ** 31 - 1, -2 ** 31
    env = make_env(scenes, N, M, omega)
    out = env.teacher_steps(dev_i32(start, env))
    torch.cuda.synchronize()
    act, steps, stats = out["actions"].cpu().numpy(), out["steps"].cpu().numpy(), out["stats"].cpu().numpy()
    assigned = env.assigned.cpu().numpy()
    for e, (sc, a) in enumerate(zip(scenes, start)):
        want = teacher_np(sc, a, omega)
        teach, invalid = teach_indices(sc["tgt_id"], a)
        n = want["steps"]
        assert steps[e] == n and np.array_equal(act[:n, e], np.array(want["actions"], np.int8)), e
        assert stats[e, 1] == invalid == want["invalid"] and stats[e, 0] == want["rejected"], e
        kept = assigned[e] >= 0
        assert np.array_equal(assigned[e][kept], np.array(teach)[kept]), e
    # more than the ids made invalid above: the ids the duplicates replaced match nothing either
    assert stats[:, 1].sum() > (bad < 0.2).sum()


def test_held_from_step_zero_and_continuation():
    """A finished env is held from step 0 (nothing changes, every row a held row); a call split in two
    (steps / ep_return accumulating) equals one call bitwise."""
    N, M, omega = 5, 7, OMEGA_REJECT
    T = N * M
    scenes = host_scenes(N, M, E)
    asg_host = random_starts(N, M, E, TEACHER_SEED)
    one = make_env(scenes, N, M, omega)
    asg = dev_i32(asg_host, one)
    full = one.teacher_steps(asg, want_info=True)
    after = state_of(one)
    # held from step 0
    again = one.teacher_steps(asg, n_max=3, want_info=True, steps=full["steps"].clone(),
                              ep_return=full["ep_return"].clone())
    torch.cuda.synchronize()
    assert_state_equal(state_of(one), after, "held")
    assert not bool(one.errors().any())
    assert torch.equal(again["steps"], full["steps"]) and torch.equal(again["ep_return"], full["ep_return"])
    assert bool(again["finished"].all()) and not bool(again["stats"][:, 0].any())
    assert not bool(again["obs"].any()) and bool((again["actions"] == -1).all()) and not bool(again["reward"].any())
    assert bool((again["done"] == 1).all()) and not bool(again["info"].any())
    # two calls
    k1 = 11
    two = make_env(scenes, N, M, omega)
    a = two.teacher_steps(asg, n_max=k1, want_info=True)
    assert not bool(a["finished"].all()) and int(a["steps"].max()) == k1
    b = two.teacher_steps(asg, n_max=T - k1, want_info=True, steps=a["steps"], ep_return=a["ep_return"])
    torch.cuda.synchronize()
    for k in ("obs", "actions", "reward", "done", "info"):
        assert torch.equal(torch.cat([a[k], b[k]]), full[k]), k
    assert torch.equal(b["steps"], full["steps"]) and torch.equal(b["ep_return"], full["ep_return"])
    assert torch.equal(b["finished"], full["finished"])
    assert torch.equal(a["stats"][:, 0] + b["stats"][:, 0], full["stats"][:, 0])
    assert_state_equal(state_of(two), after, "two calls")
    assert int(full["stats"][:, 0].sum()) > 0


def test_argument_checks():
    from uavhip import _lib
    from uavhip.vec_env import VecUAVEnv
    N, M = 4, 4
    env = make_env(host_scenes(N, M, E), N, M, 0.0)
    before = state_of(env)
    dev = env.device
    asg = torch.full((E, N), -1, dtype=torch.int32, device=dev)
    steps = torch.zeros(E, dtype=torch.int32, device=dev)
    fin = torch.zeros(E, dtype=torch.uint8, device=dev)
    fn, err = _lib.LIB.uavhip_teacher_steps, _lib.LIB.uavhip_last_error
    p = _lib.ptr

    def call(desc, a, n_max, s=steps, f=fin):
        return fn(desc, p(a), n_max, None, None, None, None, None, p(s), p(f), None, None, _lib.stream_handle())

    assert call(env.desc, asg, 0) == -1 and b"uavhip_teacher_steps" in err() and b"n_max=0" in err()
    assert call(env.desc, None, 4) == -1 and b"non-NULL" in err()
    assert call(env.desc, asg, 4, s=None) == -1 and b"non-NULL" in err()
    assert call(env.desc, asg, 4, f=None) == -1 and b"non-NULL" in err()
    half = VecUAVEnv(E, N, M, 1, 1, full_reset_period=0, obs_dtype=torch.float16)
    assert call(half.desc, asg, 4) == -1 and b"f32 observations only" in err()
    with pytest.raises(TypeError, match="f32 observations only"):
        half.teacher_steps(asg)
    with pytest.raises(ValueError, match="n_max=0"):
        env.teacher_steps(asg, n_max=0)
    with pytest.raises(ValueError, match="assignment"):
        env.teacher_steps(None)
    with pytest.raises(ValueError, match="assignment"):
        env.teacher_steps(asg.long())
    torch.cuda.synchronize()
    assert_state_equal(state_of(env), before, "refused calls")
    # every output but steps / finished is nullable: the all -1 teacher walks N * M skips
    assert call(env.desc, asg, N * M) == 0
    torch.cuda.synchronize()
    assert bool((steps == N * M).all()) and bool(fin.all()) and bool((env.assigned == -1).all())
