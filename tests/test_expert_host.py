"""Host-side checks of uavhip_expert_steps and the layers above it (no GPU): expert_np, the restatement
of the state-wise expert rule (include/uavhip.h) in Python floats driving the oracle env, that
tests/test_gpu_expert.py compares the kernel against; its follow walk against one best-response sweep
(refine_np, tests/test_refine_host.py); the conditions the GPU cases rely on, shown on the oracle's
tables; the entry point's argument checks; the binding's and ImitationRun's refusals."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import capi_host
from test_refine_host import RTOL_J, SHAPES, _env_desc, host_scenes, prm, refine_np

CASES = SHAPES + [(8, 128, 4)]      # (N, M, E); the last two: two targets per lane
OMEGAS_FOLLOW = (0.0, 0.5, 2.0)
FLIP_P, FLIP_SEED = 0.1, 11         # the relabel traces: the expert's walk, each action flipped with FLIP_P


def gpu_cases():
    """(N, M, E, omega) of tests/test_gpu_expert.py: every shape at omega 0 and 0.5, 16 x 32 also at 2."""
    out = [(N, M, E, w) for (N, M, E), w in itertools.product(CASES, (0.0, 0.5))]
    return out + [(16, 32, 32, 2.0)]


_entry_point = capi_host._entry_point("uavhip_expert_steps")


def expert_np(scene, omega, trace=None, tables=None, flip=None):
    """uavhip_expert_steps for one scene from a reset, in Python floats (IEEE doubles, one rounding per
    operation, nothing contracted): the label and margin of the rule at the oracle env's pointer
    (uav_idx / target_idx) and locks (assigned()), the step by the oracle env.
    trace: the actions to take (None: follow the labels); a value outside {0, 1} while the env is
    live ends the walk there (ended = 1). flip = (rng, p): follow, each action flipped with
    probability p. tables = (p_dmg [N, M], p_pen [N]) the rule reads (None: the oracle's own).
    -> dict: actions, labels, margins, rewards, dones (lists over the steps taken), steps, rejected,
    differ, ended, finished, assigned (target ids), J (the last info's), ep_return (rewards summed in
    step order)."""
    import oracle
    p = prm(omega)
    pd, pp = oracle.score_pairs(scene, p) if tables is None else tables
    N, M = np.shape(pd)
    P = [[float(pd[u][t]) * float(pp[u]) for t in range(M)] for u in range(N)]
    v, c, w = [float(x) for x in scene["tgt_value"]], [float(x) for x in scene["uav_cost"]], float(omega)
    ids = [int(i) for i in scene["tgt_id"]]
    env = oracle.OracleEnv(scene, p)
    env.reset()
    out = dict(actions=[], labels=[], margins=[], rewards=[], dones=[], rejected=0, differ=0, ended=0, ep_return=0.0,
               J=0.0)
    done = False
    while not done:
        u, t = env.uav_idx, env.target_idx
        lock = [ids.index(int(i)) if i >= 0 else -1 for i in env.assigned()]
        Q = [1.0] * M
        for x in range(N):  # ascending x, from 1.0
            if lock[x] >= 0:
                Q[lock[x]] = Q[lock[x]] * (1.0 - P[x][lock[x]])
        g = [(v[s] * Q[s]) * P[u][s] - (w * c[u]) for s in range(M)]
        label = int(g[t] > 0.0 and all(g[s] <= g[t] for s in range(t + 1, M)))
        margin = g[t] - max([0.0] + g[t + 1:])
        if trace is None:
            a = label
            if flip is not None and flip[0].random() < flip[1]:
                a = 1 - a
        else:
            a = int(trace[len(out["actions"])]) if len(out["actions"]) < len(trace) else -1
            if a not in (0, 1):
                out["ended"] = 1
                break
        _, r, done, info = env.step(a)
        if a == 1 and env.assigned()[u] == -1:
            out["rejected"] += 1
        out["differ"] += a != label
        for k, x in zip(("actions", "labels", "margins", "rewards", "dones"), (a, label, margin, r, int(done))):
            out[k].append(x)
        out["ep_return"] = out["ep_return"] + r
        out["J"] = float(info[0])
    out["steps"], out["finished"], out["assigned"] = len(out["actions"]), int(done), env.assigned()
    return out


@functools.lru_cache(maxsize=None)
def flipped_traces(N, M, E, omega):
    """The relabel traces of one case, on the oracle's tables: per env, the expert's walk with each
    action flipped with probability FLIP_P (one host rng per case, envs in order). -> tuple of
    expert_np results; r["actions"] is the trace."""
    rng = np.random.default_rng(FLIP_SEED)
    return tuple(expert_np(sc, omega, flip=(rng, FLIP_P)) for sc in host_scenes(N, M, E))


def trace_array(runs, T):
    """[T, E] int8: every env's trace, -1 past its end (uavhip_decode_steps' convention)."""
    a = np.full((T, len(runs)), -1, np.int8)
    for e, r in enumerate(runs):
        a[:r["steps"], e] = r["actions"]
    return a


@pytest.mark.parametrize("omega", OMEGAS_FOLLOW)
@pytest.mark.parametrize("N,M,E", CASES)
def test_follow_walk_is_one_best_response_sweep(N, M, E, omega):
    """Following the labels from a reset ends on refine_np(start=None, max_sweeps=1)'s allocation, J to
    the reward bar (the env sums J over the targets in list order, the search likewise: rounding only);
    the env rejects no assign, every action is the label, and the walk has
    sum_u (a[u] >= 0 ? a[u] + 1 : M) steps."""
    import oracle
    worst = 0.0
    for sc in host_scenes(N, M, E):
        pd, pp = oracle.score_pairs(sc, prm(omega))
        got = expert_np(sc, omega)
        want, J, _, st, _, _ = refine_np(pd, pp, sc["tgt_value"], sc["uav_cost"], sc["tgt_id"], omega, None, 1)
        assert np.array_equal(got["assigned"], want)
        assert got["rejected"] == 0 and got["differ"] == 0 and got["finished"] == 1 and got["ended"] == 0
        assert got["actions"] == got["labels"] and sum(got["actions"]) == int((want >= 0).sum()) == st[1]
        ids = [int(i) for i in sc["tgt_id"]]
        assert got["steps"] == sum(ids.index(int(i)) + 1 if i >= 0 else M for i in want)
        worst = max(worst, abs(got["J"] - J) / max(1.0, abs(J)))
        # the margin's sign is the label (IEEE subtraction keeps the sign of a difference; 0 is a tie)
        assert all(m >= 0.0 if l == 1 else m <= 0.0 for m, l in zip(got["margins"], got["labels"]))
    print(f"({N}, {M}, {E}) omega {omega}: max J err vs one sweep {worst:.2e} (bar {RTOL_J:g})")
    assert worst <= RTOL_J


@pytest.mark.parametrize("N,M,E,omega", gpu_cases())
def test_trace_conditions(N, M, E, omega):
    """What the GPU relabel cases rely on: every case has label-1 rows, label-0 rows and steps whose
    action differs from the label; at omega > 0 the env rejects at least one assign."""
    runs = flipped_traces(N, M, E, omega)
    ones = sum(sum(r["labels"]) for r in runs)
    rows = sum(r["steps"] for r in runs)
    differ = sum(r["differ"] for r in runs)
    rejected = sum(r["rejected"] for r in runs)
    print(f"({N}, {M}, {E}) omega {omega}: {rows} rows, {ones} label-1, {differ} differ, {rejected} rejected")
    assert ones > 0 and rows - ones > 0 and differ > 0
    assert all(r["finished"] == 1 and r["ended"] == 0 and N <= r["steps"] <= N * M for r in runs)
    assert omega == 0.0 or rejected > 0
    # replaying a trace gives the walk that made it; cut short, it ends the trace on a live env
    again = expert_np(host_scenes(N, M, E)[0], omega, trace=runs[0]["actions"])
    assert all(again[k] == runs[0][k] for k in ("actions", "labels", "margins", "rewards", "steps", "differ"))
    cut = expert_np(host_scenes(N, M, E)[0], omega, trace=runs[0]["actions"][:N - 1] + [-1])
    assert cut["ended"] == 1 and cut["finished"] == 0 and cut["steps"] == N - 1


def test_binding_signature():
    from uavhip import _lib
    res, args = _lib._SIGS["uavhip_expert_steps"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), vp, vp, i32] + [vp] * 11
    assert _lib.LIB.uavhip_expert_steps.argtypes == args


def test_expert_argument_checks_without_gpu():
    """Every documented misuse returns UAVHIP_EINVAL with a message naming the function, before any
    HIP call (the placeholder pointers would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_expert_steps, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_expert_steps"

    def call(env=None, act=P, follow=P, n_max=4, steps=P, fin=P):
        return fn(env or _env_desc(), act, follow, n_max, P, P, P, P, P, P, steps, fin, P, P, None)

    assert call(n_max=0) == -1 and name in err() and b"n_max=0" in err()
    assert call(n_max=-3) == -1 and name in err() and b"n_max=-3" in err()
    assert call(steps=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(fin=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(act=None) == -1 and name in err() and b"follow needs actions_in" in err()
    f16 = _env_desc()
    f16.flags = _lib.ENV_OBS_F16
    assert call(env=f16) == -1 and name in err() and b"f32 observations only" in err()
    assert call(env=_env_desc(N=65)) == -1 and name in err() and b"bad env dims" in err()
    assert call(env=_env_desc(M=129)) == -1 and name in err() and b"bad env dims" in err()
    assert call(env=_env_desc(N=0)) == -1 and name in err()
    assert fn(None, P, P, 1, P, P, P, P, P, P, P, P, P, P, None) == -1 and name in err()


class _HostEnv:
    """VecUAVEnv.expert_steps' checks run before any device call: a stand-in with the attributes they read."""

    def __init__(self, E, N, M, obs_dtype=None):
        import torch
        self.E, self.N, self.M, self.device = E, N, M, torch.device("cpu")
        self.obs_dtype = torch.float32 if obs_dtype is None else obs_dtype


def test_binding_refusals():
    import torch

    from uavhip.vec_env import VecUAVEnv
    E, N, M = 6, 4, 4
    env = _HostEnv(E, N, M)
    call = lambda *a, **k: VecUAVEnv.expert_steps(env, *a, **k)  # noqa: E731
    trace = torch.zeros(N * M, E, dtype=torch.int8)
    with pytest.raises(TypeError, match="f32 observations only"):
        VecUAVEnv.expert_steps(_HostEnv(E, N, M, torch.float16))
    with pytest.raises(ValueError, match="follow needs actions"):
        call(None, torch.zeros(E, dtype=torch.uint8))
    with pytest.raises(ValueError, match="n_max=0"):
        call(n_max=0)
    with pytest.raises(ValueError, match=r"actions must be an \[n_max, E\] int8 tensor"):
        call(trace.reshape(-1))
    with pytest.raises(ValueError, match="actions: need a contiguous torch.int8"):
        call(trace.long())
    with pytest.raises(ValueError, match="actions: need a contiguous torch.int8"):
        call(trace[:, :E - 1])
    with pytest.raises(ValueError, match="actions: need a contiguous torch.int8"):
        call(trace, n_max=N * M - 1)  # the trace must be exactly n_max rows
    with pytest.raises(ValueError, match="follow: need a contiguous torch.uint8"):
        call(trace, torch.zeros(E, dtype=torch.int8))
    with pytest.raises(ValueError, match="follow: need a contiguous torch.uint8"):
        call(trace, torch.zeros(E + 1, dtype=torch.uint8))
    for name, bad in (("labels", torch.zeros(N * M, E, dtype=torch.uint8)), ("margin", torch.zeros(N * M, E)),
                      ("stats", torch.zeros(E, 2, dtype=torch.int32)), ("steps", torch.zeros(E, dtype=torch.int64)),
                      ("obs", torch.zeros(N * M, E, 5, 14, dtype=torch.float16)),
                      ("actions_out", torch.zeros(N * M + 1, E, dtype=torch.int8))):
        with pytest.raises(ValueError, match=name + ": need a contiguous"):
            call(trace, **{name: bad})


def test_imitation_run_source_validation(tmp_path, monkeypatch):
    import torch

    from uavhip import imitate

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    out = str(tmp_path / "o")
    for kw, word in ((dict(source="dagger", targets=70), "dagger"), (dict(source="dagger", uavs=4, targets=65), "dagger"),
                     (dict(source="student"), "source='student'"), (dict(source="dagger", expert_share=1.5), "expert_share=1.5"),
                     (dict(source="dagger", expert_share=-0.1), "expert_share=-0.1")):
        args = dict(envs=64, uavs=4, targets=4, minibatch=64, out_dir=out)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            imitate.ImitationRun(**args)
    assert not (tmp_path / "o").exists()
    # "expert" has no decode limit: the arguments pass, and only then is the device asked for
    with pytest.raises(AssertionError, match="a device was touched"):
        imitate.ImitationRun(envs=64, uavs=4, targets=70, minibatch=64, out_dir=out, source="expert")
    assert not (tmp_path / "o").exists()
    assert imitate.SOURCES == ("teacher", "expert", "dagger")
    with pytest.raises(SystemExit):
        imitate.main(["--iterations", "1", "--out", out, "--source", "student"])
