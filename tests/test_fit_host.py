"""CPU-only checks of the training driver (uavhip/fit.py) and of the diagnostics entry point's
host side: the ctypes mirror against the header, the argument checks that run before any device is
touched, the state file's round trip through torch.load(weights_only=True), and the pinned progress
fields."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "uavhip.h")


def _header_enum(name):
    txt = open(HEADER).read()
    body = re.search(r"enum " + name + r" \{(.*?)\};", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out, val = {}, -1
    for item in [x.strip() for x in body.split(",") if x.strip()]:
        if "=" in item:
            k, v = [y.strip() for y in item.split("=")]
            val = int(v)
        else:
            k = item
            val += 1
        out[k] = val
    return out


def test_ctypes_mirrors_the_diagnostics_entry_point():
    from uavhip import _lib
    assert hasattr(_lib.LIB, "uavhip_ppo_diagnostics") and "uavhip_ppo_diagnostics" in _lib.EXPORTS
    assert "uavhip_ppo_diagnostics_partials" in _lib.EXPORTS
    h = _header_enum("uavhip_diag")
    assert h.pop("UAVHIP_DIAG_COUNT") == _lib.DIAG_COUNT == len(_lib.DIAG)
    assert h == {"UAVHIP_DIAG_" + k: v for k, v in _lib.DIAG.items()}
    for k in ("APPROX_KL", "CLIP_FRAC", "RATIO_MAX", "RATIO_MEAN", "VALUE_CLIP_FRAC", "EXPLAINED_VAR", "NONFINITE"):
        assert k in _lib.DIAG
    # the signature in the header: five f32 arrays, n, eps_clip, partials + its size, out, stream
    txt = open(HEADER).read()
    sig = re.search(r"int uavhip_ppo_diagnostics\((.*?)\);", txt, re.S).group(1)
    kinds = [re.sub(r"\s+\w+$", "", a.strip()) for a in sig.split(",")]
    assert kinds == ["const float*"] * 5 + ["int64_t", "double", "double*", "int32_t", "double*", "uavhip_stream_t"]
    res, args = _lib._SIGS["uavhip_ppo_diagnostics"]
    vp = ctypes.c_void_p
    assert res is ctypes.c_int
    assert args == [vp] * 5 + [ctypes.c_int64, ctypes.c_double, vp, ctypes.c_int32, vp, vp]


def test_diagnostics_argument_checks_without_gpu():
    """n >= 1, every pointer non-NULL and a large enough partials buffer, each refused with
    UAVHIP_EINVAL and a message before any HIP call."""
    from uavhip import _lib
    L = _lib.LIB
    p = ctypes.c_void_p(16)  # non-NULL placeholder: validation never dereferences it
    eps = ctypes.c_double(0.2)
    assert L.uavhip_ppo_diagnostics(p, p, p, p, p, 0, eps, p, 1 << 20, p, None) == -1
    assert b"n=0" in L.uavhip_last_error()
    for hole in range(5):
        arr = [p] * 5
        arr[hole] = None
        assert L.uavhip_ppo_diagnostics(*arr, 4, eps, p, 1 << 20, p, None) == -1
        assert b"NULL pointer" in L.uavhip_last_error()
    assert L.uavhip_ppo_diagnostics(p, p, p, p, p, 4, eps, None, 1 << 20, p, None) == -1
    assert L.uavhip_ppo_diagnostics(p, p, p, p, p, 4, eps, p, 1 << 20, None, None) == -1
    need = L.uavhip_ppo_diagnostics_partials(8209)
    assert need > L.uavhip_ppo_diagnostics_partials(1) > 0 and L.uavhip_ppo_diagnostics_partials(0) == -1
    assert L.uavhip_ppo_diagnostics_partials(1 << 40) == L.uavhip_ppo_diagnostics_partials(1 << 30)  # capped
    assert L.uavhip_ppo_diagnostics(p, p, p, p, p, 8209, eps, p, need - 1, p, None) == -1
    assert b"partials" in L.uavhip_last_error()


@pytest.mark.parametrize("kw, name", [
    (dict(envs=64, uavs=4, targets=4, horizon=16, minibatch=100), "minibatch"),
    (dict(envs=4, uavs=4, targets=4, horizon=16, minibatch=128), "minibatch"),
    (dict(envs=64, uavs=65, targets=4, horizon=16, minibatch=256, eval_every=1), "eval_every"),
    (dict(envs=64, uavs=4, targets=100, horizon=16, minibatch=256, eval_every=2), "eval_every"),
])
def test_training_run_rejects_bad_shapes_before_any_device(kw, name, tmp_path, monkeypatch):
    from uavhip import fit

    def no_device(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    out = tmp_path / "run"
    with pytest.raises(ValueError, match=name):
        fit.TrainingRun(out_dir=str(out), **kw)
    assert not out.exists()  # nothing was created either
    if name == "minibatch" and kw["minibatch"] == 128:
        with pytest.raises(ValueError, match=r"horizon \* envs"):
            fit.TrainingRun(out_dir=str(out), **kw)


def _cpu_state(fit, envs=8):
    g = torch.Generator().manual_seed(3)
    hyper = dict(envs=envs, uavs=4, targets=4, horizon=16, minibatch=64, seed=3, epochs=5, target_kl=float("nan"),
                 reset_episodes=200, lr_actor=2e-4, lr_critic=1e-3, eps_clip=0.2, max_grad_norm=1.0, value_coef=0.5,
                 entropy_coef=0.01, gamma=0.998, gae_lambda=0.95)
    s = {"format": fit.STATE_FORMAT, "run.iteration": 2, "run.best": float("-inf"), "run.wall_s": 1.5,
         "engine.iteration": 2, "env.seed": 2 ** 63 + 5, "env.flags": 0,
         "trainer.params": torch.randn(1000, generator=g), "trainer.adam_step": torch.tensor([10.0], dtype=torch.float64),
         "engine.counter": torch.tensor([2 * 17 * envs], dtype=torch.int64),
         "env.istate": torch.randint(0, 9, (envs, 12), generator=g, dtype=torch.int32),
         "env.dstate": torch.randn(envs, 12, generator=g, dtype=torch.float64),
         "env.scene.uav_type": torch.randint(0, 2, (2 * envs, 4), generator=g, dtype=torch.int32),
         "stats.acc": torch.randn(envs, 12, generator=g, dtype=torch.float64),
         "generator.state": g.get_state().clone()}
    s.update({"hp." + k: v for k, v in hyper.items()})
    return s, hyper


def test_state_survives_a_weights_only_round_trip(tmp_path):
    from uavhip import fit
    s, hyper = _cpu_state(fit)
    path = str(tmp_path / "state_it2.pt")
    fit.save_state(s, path)
    assert not os.path.exists(path + ".tmp")
    back = torch.load(path, map_location="cpu", weights_only=True)  # nothing in the file is executed
    assert list(back) == list(s)
    for k, v in s.items():
        if isinstance(v, torch.Tensor):
            assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
        elif isinstance(v, float) and math.isnan(v):
            assert math.isnan(back[k]), k
        else:
            assert back[k] == v and type(back[k]) is type(v), k
    assert fit.load_state(path).keys() == s.keys()
    fit.check_compatible(back, hyper)  # the same shape and hyper-parameters: accepted
    # the generator continues from the restored state
    g1, g2 = torch.Generator(), torch.Generator()
    g1.set_state(s["generator.state"])
    g2.set_state(back["generator.state"])
    assert torch.equal(torch.randperm(50, generator=g1), torch.randperm(50, generator=g2))
    with pytest.raises(TypeError, match="run.list"):
        fit.save_state(dict(s, **{"run.list": [1, 2]}), path)  # flat: tensors, ints, floats, strings only
    # a run directory resolves to its latest state
    fit.save_state(s, str(tmp_path / "state_it10.pt"))
    assert fit.latest_state(str(tmp_path)).endswith("state_it10.pt")
    assert fit.latest_state(path) == path


@pytest.mark.parametrize("field, value", [("envs", 16), ("horizon", 32), ("minibatch", 128), ("lr_actor", 1e-4),
                                          ("target_kl", 0.02), ("seed", 4)])
def test_a_state_of_another_shape_is_refused_by_name(field, value, tmp_path, monkeypatch):
    from uavhip import fit
    s, hyper = _cpu_state(fit)
    with pytest.raises(ValueError, match=rf"resume: {field} differs"):
        fit.check_compatible(s, dict(hyper, **{field: value}))
    if field in ("envs", "horizon", "minibatch", "seed"):
        # through the constructor: refused while reading the state, before any device is touched
        def no_device(*a, **k):
            raise AssertionError("a device was touched before the state was checked")
        monkeypatch.setattr(torch.cuda, "is_available", no_device)
        path = str(tmp_path / "state_it2.pt")
        fit.save_state(s, path)
        kw = dict(envs=8, uavs=4, targets=4, horizon=16, minibatch=64, seed=3)
        kw[field] = value
        with pytest.raises(ValueError, match=rf"resume: {field} differs"):
            fit.TrainingRun(out_dir=str(tmp_path / "o"), resume=str(tmp_path), **kw)


def test_progress_fields_are_pinned():
    from uavhip import _lib, fit
    assert fit.PROGRESS_FIELDS == ("iteration", "env_steps", "episodes", "mean_ep_reward", "mean_ep_steps",
                                   "mean_ep_J", "loss_actor", "loss_critic", "entropy", "epochs_run",
                                   "optimizer_steps", "wall_s", "env_steps_per_s")
    assert fit.DIAG_FIELDS == tuple(k.lower() for k, _ in sorted(_lib.DIAG.items(), key=lambda kv: kv[1]))
    assert fit.EVAL_FIELDS == ("eval_mean_J", "eval_mean_J_baseline", "eval_beats_baseline")
    line = fit.progress_line({"iteration": 1, "mean_ep_reward": float("nan"), "explained_var": float("inf"),
                              "entropy": 0.5})
    assert json.loads(line) == {"iteration": 1, "mean_ep_reward": None, "explained_var": None, "entropy": 0.5}
    assert "NaN" not in line and "Infinity" not in line
