"""Host side of the lr / entropy / clip schedules (uavhip.fit schedule_value, TrainingRun's and
FusedPPOTrainer.set_hyper's argument checks, the binding of uavhip_ppo_step_hyper and its argument
validation, check_compatible on the schedule fields). No GPU call."""
import ctypes
import math

import pytest


# ------------------------------------------------------------------ the rule
def test_schedule_value_ends():
    from uavhip.fit import schedule_value
    for kind in ("linear", "cosine"):
        for K in (2, 3, 10, 300):
            for ff in (0.0, 0.1, 0.25, 1.0 / 3.0, 1.0):
                assert schedule_value(kind, 1, K, ff) == 1.0, (kind, K, ff)
                for i in (K, K + 1, 10 * K):  # held at final_frac, exactly
                    assert schedule_value(kind, i, K, ff) == ff, (kind, K, ff, i)
    # the rule itself at an inner point: p = (i - 1) / (K - 1)
    assert schedule_value("linear", 4, 11, 0.1) == 0.1 + (1.0 - 0.1) * (1.0 - 3 / 10)
    assert schedule_value("cosine", 4, 11, 0.1) == 0.1 + (1.0 - 0.1) * (0.5 * (1.0 + math.cos(math.pi * (3 / 10))))


def test_schedule_value_cosine_midpoint():
    from uavhip.fit import schedule_value
    # K odd: i = (K + 1) / 2 is p = 0.5 exactly; cos(pi / 2) is 6e-17 in double, not 0
    for K, ff in ((3, 0.0), (101, 0.0), (101, 0.2)):
        mid = schedule_value("cosine", (K + 1) // 2, K, ff)
        assert abs(mid - (ff + (1.0 - ff) * 0.5)) <= 1e-16, (K, ff, mid)
    # above the line before the midpoint, below it after
    assert schedule_value("cosine", 26, 101, 0.0) > schedule_value("linear", 26, 101, 0.0)
    assert schedule_value("cosine", 76, 101, 0.0) < schedule_value("linear", 76, 101, 0.0)


def test_schedule_value_monotone_and_constant():
    from uavhip.fit import schedule_value
    for kind in ("linear", "cosine"):
        for W in (0, 5):
            v = [schedule_value(kind, i, 40, 0.1, W) for i in range(1, 60)]
            tail = v[W:] if W else v  # from the first iteration after the ramp
            assert all(a >= b for a, b in zip(tail, tail[1:])), (kind, W)
            assert all(0.1 <= x <= 1.0 for x in tail)
    for i in (1, 2, 17, 10 ** 6):
        assert schedule_value("constant", i, 0, 0.0) == 1.0
        assert schedule_value("constant", i, 50, 0.3) == 1.0


def test_schedule_value_warmup():
    from uavhip.fit import schedule_value
    W, K = 4, 21
    assert schedule_value("linear", 1, K, 0.0, W) == 1.0 / W
    assert schedule_value("constant", 1, 0, 0.0, W) == 1.0 / W
    for i in range(1, 12):
        base = schedule_value("linear", i, K, 0.0)
        want = base * (i / W) if i <= W else base
        assert schedule_value("linear", i, K, 0.0, W) == want
    assert schedule_value("constant", W, 0, 0.0, W) == 1.0  # the ramp ends at the full rate
    with pytest.raises(ValueError, match="kind"):
        schedule_value("step", 1, 10, 0.0)
    with pytest.raises(ValueError, match="i=0"):
        schedule_value("linear", 0, 10, 0.0)
    with pytest.raises(ValueError, match="schedule_iterations=1"):
        schedule_value("linear", 1, 1, 0.0)


def test_schedule_hyper_scales_the_base_values():
    from uavhip import fit
    hyper = dict(lr_actor=2e-4, lr_critic=1e-3, entropy_coef=0.01, eps_clip=0.2)
    sched = dict(fit.SCHEDULE_DEFAULTS, lr_schedule="linear", lr_final_frac=0.1, entropy_schedule="cosine",
                 schedule_iterations=9, lr_warmup=2)
    for i in (1, 2, 3, 9, 20):
        s_lr = fit.schedule_value("linear", i, 9, 0.1, 2)
        s_en = fit.schedule_value("cosine", i, 9, 0.0)
        got = fit.schedule_hyper(hyper, sched, i)
        assert got == dict(lr_actor=2e-4 * s_lr, lr_critic=1e-3 * s_lr, entropy_coef=0.01 * s_en, eps_clip=0.2)
    assert fit.scheduled(sched) and not fit.scheduled(fit.SCHEDULE_DEFAULTS)
    assert fit.scheduled(dict(fit.SCHEDULE_DEFAULTS, lr_warmup=3))


# ------------------------------------------------------------------ argument checks, before any device
def test_arguments_are_refused_by_name_before_any_device(tmp_path, monkeypatch):
    import torch

    from uavhip import fit
    from uavhip.train import FusedPPOTrainer, check_hyper

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    out = str(tmp_path / "o")
    args = dict(envs=64, uavs=4, targets=4, horizon=16, minibatch=64, out_dir=out)
    K = dict(schedule_iterations=10)
    bad = [
        (dict(lr_schedule="step", **K), "lr_schedule='step'"),
        (dict(entropy_schedule="exp", **K), "entropy_schedule='exp'"),
        (dict(clip_schedule="", **K), "clip_schedule=''"),
        (dict(lr_schedule="linear", lr_final_frac=1.5, **K), "lr_final_frac=1.5"),
        (dict(lr_schedule="linear", lr_final_frac=-0.1, **K), "lr_final_frac=-0.1"),
        (dict(entropy_schedule="linear", entropy_final_frac=2.0, **K), "entropy_final_frac=2.0"),
        (dict(entropy_final_frac=float("nan")), "entropy_final_frac=nan"),
        (dict(clip_schedule="linear", clip_final_frac=1.01, **K), "clip_final_frac=1.01"),
        (dict(clip_schedule="linear", clip_final_frac=0.0, **K), "clip_final_frac=0.0"),
        (dict(lr_schedule="linear"), "schedule_iterations=0"),
        (dict(lr_schedule="cosine", schedule_iterations=1), "schedule_iterations=1"),
        (dict(clip_schedule="linear", schedule_iterations=-3), "schedule_iterations=-3"),
        (dict(schedule_iterations=-1), "schedule_iterations=-1"),
        (dict(lr_warmup=-1), "lr_warmup=-1"),
        # the base values of a scheduled run pass set_hyper's checks up front (a run without a schedule
        # never calls set_hyper and takes them as before)
        (dict(lr_actor=-1e-4, lr_warmup=2), "lr_actor"),
        (dict(lr_critic=float("inf"), lr_schedule="linear", **K), "lr_critic"),
        (dict(entropy_coef=-0.01, entropy_schedule="cosine", **K), "entropy_coef"),
        (dict(eps_clip=0.0, clip_schedule="linear", clip_final_frac=0.5, **K), "eps_clip"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            fit.TrainingRun(**args, **kw)
    assert not (tmp_path / "o").exists()
    # the arguments pass, and only then is the device asked for
    with pytest.raises(AssertionError, match="a device was touched"):
        fit.TrainingRun(**args, lr_schedule="linear", lr_final_frac=0.1, entropy_schedule="cosine", lr_warmup=2, **K)
    with pytest.raises(AssertionError, match="a device was touched"):  # no schedule: the base values as before
        fit.TrainingRun(**args, eps_clip=0.0)
    with pytest.raises(SystemExit):  # the command line knows the kinds
        fit.main(["--iterations", "1", "--out", out, "--lr-schedule", "step"])
    with pytest.raises(ValueError, match="schedule_iterations=0"):
        fit.main(["--iterations", "1", "--out", out, "--envs", "64", "--uavs", "4", "--targets", "4", "--horizon",
                  "16", "--minibatch", "64", "--entropy-schedule", "linear"])

    # set_hyper: validated before the trainer's device buffer is looked at (a trainer with no
    # attributes at all: any device work would raise AttributeError instead)
    tr = object.__new__(FusedPPOTrainer)
    for kw, msg in [(dict(lr_actor=-1.0), "lr_actor must be >= 0"), (dict(lr_critic=float("nan")), "lr_critic must be finite"),
                    (dict(entropy_coef=-1e-9), "entropy_coef must be >= 0"), (dict(eps_clip=0.0), "eps_clip must be > 0"),
                    (dict(eps_clip=float("inf")), "eps_clip must be finite"), (dict(lr_actor="fast"), "lr_actor must be a number"),
                    (dict(lr_actor=1e-4, eps_clip=-0.2), "eps_clip must be > 0")]:
        with pytest.raises(ValueError, match=msg):
            tr.set_hyper(**kw)
    assert check_hyper(lr_actor=0.0, entropy_coef=0, eps_clip=0.1) == dict(lr_actor=0.0, entropy_coef=0.0, eps_clip=0.1)
    assert check_hyper() == {}


# ------------------------------------------------------------------ binding and C argument validation
def test_binding_of_step_hyper_and_abi_version():
    from uavhip import _lib
    res, args = _lib._SIGS["uavhip_ppo_step_hyper"]
    res0, args0 = _lib._SIGS["uavhip_ppo_step"]
    assert res is ctypes.c_int is res0
    # the descriptor, the hyper buffer, then exactly uavhip_ppo_step's arguments
    assert args == [args0[0], ctypes.c_void_p] + args0[1:]
    fn = _lib.LIB.uavhip_ppo_step_hyper
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == args
    assert "uavhip_ppo_step_hyper" in _lib.EXPORTS
    assert _lib.LIB.uavhip_abi_version() == _lib.ABI_VERSION == 6
    assert _lib.HP == dict(LR_ACTOR=0, LR_CRITIC=1, ENTROPY_COEF=2, EPS_CLIP=3) and _lib.HP_COUNT == 4
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "uavhip.h")).read()
    body = re.search(r"enum uavhip_ppo_hyper \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"\b(UAVHIP_HP_\w+)\b\s*(?:=\s*0)?\s*,?", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["UAVHIP_HP_LR_ACTOR", "UAVHIP_HP_LR_CRITIC", "UAVHIP_HP_ENTROPY_COEF", "UAVHIP_HP_EPS_CLIP",
                     "UAVHIP_HP_COUNT"]


def _desc(_lib):
    d = _lib.PPODesc()
    for name in ("params", "grads", "adam_m", "adam_v", "adam_step", "workspace", "loss_sums", "stats"):
        setattr(d, name, 16)  # placeholders: validation never dereferences them
    d.n_floats, d.minibatch, d.global_minibatch = _lib.LIB.uavhip_policy_layout(None, 0), 64, 64
    d.lr_actor, d.lr_critic, d.beta1, d.beta2, d.adam_eps = 2e-4, 1e-3, 0.9, 0.999, 1e-8
    d.eps_clip, d.max_grad_norm, d.value_coef, d.entropy_coef = 0.2, 1.0, 0.5, 0.01
    return d


@pytest.mark.parametrize("hyper", [None, 16])
def test_step_hyper_returns_the_steps_argument_errors_under_its_own_name(hyper):
    """Every NULL / EINVAL case of uavhip_ppo_step through the new entry point, before any HIP call
    (with and without a hyper buffer), the message naming uavhip_ppo_step_hyper."""
    from uavhip import _lib
    step = _lib.LIB.uavhip_ppo_step_hyper
    err = _lib.LIB.uavhip_last_error
    ok = (16, 16, 16, 16, 16, 16, 16, _lib.PPO_FULL, None)

    def refused(d, args, what):
        assert step(d, hyper, *args) == -1
        assert err().startswith(b"uavhip_ppo_step_hyper: " + what), err()

    refused(None, ok, b"NULL pointer")
    for name in ("params", "grads", "workspace", "loss_sums"):
        d = _desc(_lib)
        setattr(d, name, None)
        refused(d, ok, b"NULL pointer")
    for i in range(7):  # a trajectory buffer or idx missing with FORWARD / BACKWARD
        refused(_desc(_lib), ok[:i] + (None,) + ok[i + 1:], b"NULL pointer")
        refused(_desc(_lib), ok[:i] + (None,) + ok[i + 1:7] + (_lib.PPO_BACKWARD, None), b"NULL pointer")
    for field, value in (("minibatch", 0), ("minibatch", 65), ("minibatch", -64), ("global_minibatch", 32),
                         ("n_floats", 7)):
        d = _desc(_lib)
        setattr(d, field, value)
        refused(d, ok, b"minibatch")
    for phases in (0, 16, _lib.PPO_PACKED, _lib.PPO_FULL | 32):
        refused(_desc(_lib), ok[:7] + (phases, None), b"minibatch")
    for name in ("adam_m", "adam_v", "adam_step"):  # UPDATE needs the optimizer state
        d = _desc(_lib)
        setattr(d, name, None)
        refused(d, ok, b"minibatch")
    for flags in (64, 63 | 1 << 20, -1):
        d = _desc(_lib)
        d.flags = flags
        refused(d, ok, b"flags")
    # and uavhip_ppo_step keeps its own name
    assert _lib.LIB.uavhip_ppo_step(None, *ok) == -1 and err().startswith(b"uavhip_ppo_step: NULL pointer")


# ------------------------------------------------------------------ resume compatibility
def _hyper():
    return dict(envs=64, uavs=4, targets=4, horizon=16, minibatch=64, seed=0, epochs=2, target_kl=float("nan"),
                reset_episodes=10, lr_actor=2e-4, lr_critic=1e-3, eps_clip=0.2, max_grad_norm=1.0, value_coef=0.5,
                entropy_coef=0.01, gamma=0.99, gae_lambda=0.95)


def test_check_compatible_on_the_schedule_fields():
    from uavhip import fit
    assert set(fit.SCHEDULE_FIELDS) == set(fit.SCHEDULE_DEFAULTS) and not set(fit.SCHEDULE_FIELDS) & set(fit.HYPER_FIELDS)
    hyper = _hyper()
    assert set(hyper) == set(fit.HYPER_FIELDS)
    old = {"hp." + k: v for k, v in hyper.items()}  # a state from before the schedules
    fit.check_compatible(old, hyper)                                    # into a run that names no schedule
    fit.check_compatible(old, {**hyper, **fit.SCHEDULE_DEFAULTS})       # into an all-constant run
    sched = dict(fit.SCHEDULE_DEFAULTS, lr_schedule="linear", lr_final_frac=0.1, schedule_iterations=300)
    with pytest.raises(ValueError, match="lr_schedule differs.*'constant'.*'linear'"):
        fit.check_compatible(old, {**hyper, **sched})
    new = dict(old, **{"hp." + k: v for k, v in sched.items()})
    fit.check_compatible(new, {**hyper, **sched})
    with pytest.raises(ValueError, match="schedule_iterations differs.*300.*200"):
        fit.check_compatible(new, {**hyper, **dict(sched, schedule_iterations=200)})
    with pytest.raises(ValueError, match="lr_schedule differs.*'linear'.*'constant'"):
        fit.check_compatible(new, hyper)  # a scheduled state into a constant run
    for k, v in (("entropy_schedule", "cosine"), ("clip_schedule", "linear"), ("lr_final_frac", 0.2),
                 ("entropy_final_frac", 0.5), ("clip_final_frac", 0.5), ("lr_warmup", 5)):
        with pytest.raises(ValueError, match=f"resume: {k} differs"):
            fit.check_compatible(new, {**hyper, **dict(sched, **{k: v})})
    # the earlier fields are still checked first and by name
    with pytest.raises(ValueError, match="resume: lr_actor differs"):
        fit.check_compatible(new, {**dict(hyper, lr_actor=1e-4), **sched})
