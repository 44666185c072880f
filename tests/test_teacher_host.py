"""Host-side checks of uavhip_teacher_steps and the imitation layers (no GPU): the binding; teacher_np,
the restatement of the teacher-forced walk (the action rule and the pointer moves in Python, the accept
test r(X') >= r(X) by the oracle env) that tests/test_gpu_teacher.py compares the kernel against; its
closed forms at omega = 0; the conditions the GPU cases rely on, shown by the oracle alone; the entry
point's argument checks; and the argument validation of ImitationRun and of uavhip.fit --init."""
import ctypes

import numpy as np
import pytest

import capi_host
from test_refine_host import _env_desc, host_scenes, prm, random_starts

E = 64
SHAPES = [(4, 4), (5, 7), (16, 32), (33, 34), (3, 70), (8, 128)]  # the last two: two targets per lane
OMEGA_REJECT = 2.0
TEACHER_SEED = 1  # random_starts' seed: at OMEGA_REJECT every shape shows rejected assigns (checked below)


_entry_point = capi_host._entry_point("uavhip_teacher_steps")


def teach_indices(tgt_id, assignment):
    """Target ids -> list indices as the kernel converts them: the lowest list index of a duplicated
    id, an id that matches nothing counts as -1. -> (teach [N], invalid ids)."""
    ids = [int(i) for i in tgt_id]
    teach, invalid = [], 0
    for want in (int(x) for x in assignment):
        if want == -1:
            teach.append(-1)
        elif want in ids:
            teach.append(ids.index(want))
        else:
            teach.append(-1)
            invalid += 1
    return teach, invalid


def teacher_np(scene, assignment, omega):
    """uavhip_teacher_steps for one scene from a reset: a = (teach[u] == t) at the pointer (u, t), the
    step by the oracle env (its accept test, its pointer moves), until the episode ends.
    -> dict: actions, rewards, pointers [(u, t) before each step], windows [the window each action was
    decided on], steps, rejected, invalid, assigned (target ids), ep_return (rewards summed in step
    order), J (the last info's)."""
    import oracle
    teach, invalid = teach_indices(scene["tgt_id"], assignment)
    env = oracle.OracleEnv(scene, prm(omega))
    win = env.reset()
    out = dict(actions=[], rewards=[], pointers=[], windows=[], rejected=0, invalid=invalid, ep_return=0.0, J=0.0)
    done = False
    while not done:
        u, t = env.uav_idx, env.target_idx
        a = 1 if teach[u] == t else 0
        out["pointers"].append((u, t))
        out["windows"].append(win)
        win, r, done, info = env.step(a)
        if a == 1 and env.assigned()[u] == -1:
            out["rejected"] += 1
            assert r == 0.0 or done  # a rejected assign earns nothing (the goal reward aside)
        out["actions"].append(a)
        out["rewards"].append(r)
        out["ep_return"] = out["ep_return"] + r
        out["J"] = float(info[0])
    out["steps"] = len(out["actions"])
    out["assigned"] = env.assigned()
    return out


def closed_form_steps(teach, M):
    return sum(t + 1 if t >= 0 else M for t in teach)


def test_binding_signature():
    from uavhip import _lib
    res, args = _lib._SIGS["uavhip_teacher_steps"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    assert _lib.LIB.uavhip_teacher_steps.argtypes == args
    assert _lib.ABI_VERSION == 6 and _lib.LIB.uavhip_abi_version() == 6


@pytest.mark.parametrize("N,M", SHAPES[:4] + [(3, 70)])
def test_closed_forms_at_omega_zero(N, M):
    """omega = 0 and values >= 0: J never falls and no target is uncovered by an assign, so every
    teacher assign is accepted: the env ends on the teacher's allocation after
    sum_u (teach[u] >= 0 ? teach[u] + 1 : M) steps."""
    n = 6
    scenes = host_scenes(N, M, E)[:n]
    starts = random_starts(N, M, E, TEACHER_SEED)[:n]
    for sc, a in zip(scenes, starts):
        assert float(np.min(sc["tgt_value"])) >= 0
        got = teacher_np(sc, a, 0.0)
        teach, invalid = teach_indices(sc["tgt_id"], a)
        assert invalid == 0 and got["rejected"] == 0
        assert np.array_equal(got["assigned"], a)
        assert got["steps"] == closed_form_steps(teach, M) and N <= got["steps"] <= N * M
        assert sum(got["actions"]) == sum(t >= 0 for t in teach)


def test_rejection_case_shows_rejections_on_the_oracle():
    """The GPU rejection test's cases (random teacher, omega = 2) reject assigns in every shape, by the
    oracle alone; a rejected UAV stays unassigned."""
    for N, M in SHAPES:
        n = 8 if N * M > 600 else 24
        scenes = host_scenes(N, M, E)[:n]
        starts = random_starts(N, M, E, TEACHER_SEED)[:n]
        rej = 0
        for sc, a in zip(scenes, starts):
            got = teacher_np(sc, a, OMEGA_REJECT)
            rej += got["rejected"]
            kept = got["assigned"] >= 0
            assert np.array_equal(got["assigned"][kept], a[kept])
            assert int((a >= 0).sum()) - int(kept.sum()) == got["rejected"]
        print(f"({N}, {M}): {rej} rejected teacher assigns in {n} scenes")
        assert rej > 0, (N, M)


def test_invalid_and_duplicated_ids():
    N, M = 5, 7
    sc = dict(host_scenes(N, M, 1)[0])
    ids = sc["tgt_id"].copy()
    ids[M - 1] = ids[0]  # a duplicated id: the lowest list index is meant; the id it replaced is gone
    gone = int(sc["tgt_id"][M - 1])
    sc["tgt_id"] = ids
    a = np.array([int(ids[0]), 99, -1, -7, gone], np.int32)
    teach, invalid = teach_indices(ids, a)
    assert teach == [0, -1, -1, -1, -1] and invalid == 3
    got = teacher_np(sc, a, 0.0)
    assert got["invalid"] == 3 and got["steps"] == 1 + 4 * M and sum(got["actions"]) == 1


def test_teacher_argument_checks_without_gpu():
    """Every documented misuse returns UAVHIP_EINVAL with a message naming the function, before any
    HIP call (the placeholder pointers would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_teacher_steps, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_teacher_steps"

    def call(env=None, asg=P, n_max=4, steps=P, fin=P):
        return fn(env or _env_desc(), asg, n_max, P, P, P, P, P, steps, fin, P, P, None)

    assert call(n_max=0) == -1 and name in err() and b"n_max=0" in err()
    assert call(n_max=-3) == -1 and name in err() and b"n_max=-3" in err()
    assert call(asg=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(steps=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(fin=None) == -1 and name in err() and b"non-NULL" in err()
    f16 = _env_desc()
    f16.flags = _lib.ENV_OBS_F16
    assert call(env=f16) == -1 and name in err() and b"f32 observations only" in err()
    assert call(env=_env_desc(N=65)) == -1 and name in err() and b"bad env dims" in err()
    assert call(env=_env_desc(M=129)) == -1 and name in err() and b"bad env dims" in err()
    assert fn(None, P, 1, P, P, P, P, P, P, P, P, P, None) == -1 and name in err()


def test_init_with_resume_is_refused_before_any_device(tmp_path, monkeypatch):
    import torch

    from uavhip import fit

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(ValueError, match="init and resume exclude each other"):
        fit.TrainingRun(64, 4, 4, 8, 64, str(tmp_path / "o"), init=str(tmp_path / "m.pth"), resume=str(tmp_path / "r"))
    with pytest.raises(ValueError, match="init and resume exclude each other"):
        fit.main(["--iterations", "1", "--out", str(tmp_path / "o"), "--init", "m.pth", "--resume", "r"])
    assert not (tmp_path / "o").exists()
    assert "init" not in fit.HYPER_FIELDS


def test_imitation_run_argument_validation(tmp_path, monkeypatch):
    import torch

    from uavhip import imitate

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    out = str(tmp_path / "o")
    for kw, word in ((dict(minibatch=100), "minibatch=100"), (dict(minibatch=0), "minibatch=0"),
                     (dict(envs=0), "envs=0"), (dict(uavs=65), "uavs=65"), (dict(targets=129), "targets=129"),
                     (dict(epochs=0), "epochs=0"), (dict(eval_every=-1), "eval_every=-1"),
                     (dict(targets=70, eval_every=1), "eval_every=1")):
        args = dict(envs=64, uavs=4, targets=4, minibatch=64, out_dir=out)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            imitate.ImitationRun(**args)
    assert not (tmp_path / "o").exists()
    with pytest.raises(SystemExit):
        imitate.main(["--out", out])  # --iterations is required
    assert imitate.PROGRESS_FIELDS == ("iteration", "rows", "nll_before", "nll_after", "agreement", "teacher_mean_J",
                                       "rejected")
