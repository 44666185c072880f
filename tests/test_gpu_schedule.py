"""The scheduled hyper-parameters on the GPU: uavhip_ppo_step_hyper reads the learning rates, the
entropy coefficient and the clip range from device memory (csrc/train.hip adam_advance, csrc/policy.hip
heads_bwd, csrc/policy_block.hpp loss_partials), FusedPPOTrainer.set_hyper feeds it and keeps the
captured epoch graph, and uavhip.fit drives it from schedule_value. Marked gpu.

Every comparison is bitwise: the by-value step (uavhip_ppo_step on a descriptor holding the values) runs
the same kernels on the same numbers -- (float)(double)f == f for the two float fields, the learning
rates are doubles on both sides -- so there is no tolerance to choose. Each kernel path of the step gets
one minibatch size: 64 (position split), 64 with the position split off (K6, trunk-split), 1024
(trunk-split, above the position split's range), 4096 (both trunks in every workgroup)."""
import copy
import json
import os

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

NAMES = ("params", "adam_m", "adam_v", "adam_step", "grads", "loss_sums", "stats")
DEFAULT = dict(lr_actor=2e-4, lr_critic=1e-3, entropy_coef=0.01, eps_clip=0.2)
OTHER = dict(lr_actor=1e-4, lr_critic=5e-4, entropy_coef=0.03, eps_clip=0.1)  # lr x 0.5, entropy 0.03, clip 0.1
STEPS = 3


def _paths():
    from uavhip import _lib
    return [pytest.param(64, 0, id="64-pos-split"), pytest.param(64, _lib.PPO_NO_POS_SPLIT, id="64-k6-trunk-split"),
            pytest.param(1024, 0, id="1024-trunk-split"), pytest.param(4096, 0, id="4096-fused-trunks")]


def _buffers(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    states = torch.randn(n, 5, 14, generator=g) * 0.5
    states[: n // 3, :2] = 0          # padded windows (masked keys)
    states[n // 3: n // 2, :4] = 0    # only the current step
    acts = torch.randint(0, 2, (n,), generator=g)
    logp = -0.69 + 0.15 * torch.randn(n, generator=g)   # ratios on both sides of 1 +- 0.1 and 1 +- 0.2
    vals = torch.randn(n, generator=g)
    ret = vals + 0.3 * torch.randn(n, generator=g)
    vals = vals + 0.15 * torch.randn(n, generator=g)    # new - old values on both sides of 0.1 and 0.2
    adv = torch.randn(n, generator=g)
    return [t.cuda() for t in (states, acts, logp, vals, ret, adv)]


def _state(tr):
    torch.cuda.synchronize()
    return {k: getattr(tr, k).detach().clone() for k in NAMES}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _assert_same(got, want, label):
    for k in NAMES:
        assert _same(got[k], want[k]), f"{label}: {k}: {int((got[k] != want[k]).sum())} elements differ"


class _Case:
    """One kernel path: the model, the buffers, the minibatch order, and the by-value results, each
    computed once and shared by the tests (never modified)."""

    def __init__(self, Bm, flags):
        from uavhip.policy import TransformerActorCritic
        self.Bm, self.flags = Bm, flags
        torch.manual_seed(100 + Bm + flags)
        self.base = TransformerActorCritic().cuda()
        self.bufs = _buffers(STEPS * Bm, seed=200 + Bm)
        self.perm = torch.randperm(STEPS * Bm, generator=torch.Generator().manual_seed(300 + Bm)).to(torch.int32).cuda()
        self._by_value = {}

    def trainer(self, values=None, **kw):
        from uavhip.train import FusedPPOTrainer
        tr = FusedPPOTrainer(copy.deepcopy(self.base), self.Bm, flags=self.flags, **(values or {}), **kw)
        tr.set_buffers(*self.bufs)
        return tr

    def rows(self, b):
        return self.perm[b * self.Bm:(b + 1) * self.Bm]

    def full_steps(self, tr):
        from uavhip import _lib
        for b in range(STEPS):
            tr.step(_lib.PPO_FULL | tr._packed(b), self.rows(b))
        return _state(tr)

    def by_value(self, key):
        """STEPS FULL steps of uavhip_ppo_step on a descriptor holding DEFAULT / OTHER."""
        if key not in self._by_value:
            tr = self.trainer(dict(DEFAULT=DEFAULT, OTHER=OTHER)[key])
            assert tr.hyper is None
            self._by_value[key] = self.full_steps(tr)
        return self._by_value[key]


_CASES = {}


def _case(Bm, flags):
    if (Bm, flags) not in _CASES:
        _CASES[(Bm, flags)] = _Case(Bm, flags)
    return _CASES[(Bm, flags)]


@pytest.mark.parametrize("Bm,flags", _paths())
def test_hyper_buffer_with_the_descriptors_values_is_the_by_value_step(Bm, flags):
    """set_hyper() with no value: the buffer holds the descriptor's own values. Three FULL steps of
    uavhip_ppo_step_hyper == three of uavhip_ppo_step, bitwise in everything the step writes."""
    c = _case(Bm, flags)
    tr = c.trainer()
    tr.set_hyper()
    assert tr.hyper is not None and tr.hyper.dtype == torch.float64 and tr.hyper.numel() == 4
    d = tr.desc  # the two float fields widened to double
    assert tr.hyper.tolist() == [d.lr_actor, d.lr_critic, float(d.entropy_coef), float(d.eps_clip)]
    assert [d.lr_actor, d.lr_critic, d.entropy_coef, d.eps_clip] == pytest.approx(list(DEFAULT.values()), rel=1e-7)
    _assert_same(c.full_steps(tr), c.by_value("DEFAULT"), "descriptor's values from the buffer")


@pytest.mark.parametrize("Bm,flags", _paths())
def test_other_values_from_the_buffer_are_the_by_value_step_on_them(Bm, flags):
    """lr x 0.5, entropy 0.03, clip 0.1 in the buffer, the defaults in the descriptor: bitwise the
    by-value step on a descriptor holding those values -- and not the default-valued step (the
    gradients through the entropy and clip terms, the parameters through the learning rates too), so
    this is not a comparison of two paths that both ignore the values."""
    c = _case(Bm, flags)
    tr = c.trainer()  # the descriptor keeps the defaults: ignored in this mode
    tr.set_hyper(**OTHER)
    got = c.full_steps(tr)
    assert [tr.desc.lr_actor, tr.desc.lr_critic] == [2e-4, 1e-3]
    _assert_same(got, c.by_value("OTHER"), "other values from the buffer")
    dflt = c.by_value("DEFAULT")
    for k in ("params", "grads", "loss_sums", "adam_m", "adam_v"):
        assert not _same(got[k], dflt[k]), f"{k} equals the default-valued step's"
    assert _same(got["adam_step"], dflt["adam_step"])


def test_each_value_reaches_its_kernels():
    """One value changed at a time (minibatch 64, FORWARD | BACKWARD then UPDATE): the clip range
    changes the forward's loss sums and the gradients, the entropy coefficient the gradients alone,
    the learning rates neither -- they change the parameters, the actor's rate the actor's (below the
    critic trunk's offset) and the critic's rate the rest."""
    from uavhip import _lib
    from uavhip.policy import layout
    c = _case(64, 0)
    out = {}
    for name in ("none", "lr_actor", "lr_critic", "entropy_coef", "eps_clip"):
        tr = c.trainer()
        tr.set_hyper(**({} if name == "none" else {name: OTHER[name]}))
        tr.step(_lib.PPO_FORWARD | _lib.PPO_BACKWARD, c.rows(0))
        raw = tr.grads.clone()
        tr.step(_lib.PPO_UPDATE, c.rows(0))
        torch.cuda.synchronize()
        out[name] = (tr.loss_sums.clone(), raw, tr.params.clone())
    l0, g0, p0 = out["none"]
    offs, _ = layout()
    names = list(c.base.state_dict())
    first = next(i for i, k in enumerate(names) if k.startswith("critic"))
    assert all(k.startswith("actor") for k in names[:first]) and all(k.startswith("critic") for k in names[first:])
    crit = offs[first]
    l, g, p = out["eps_clip"]
    assert not _same(l, l0) and not _same(g, g0)
    assert _same(l[3:], l0[3:])  # the entropy sum does not depend on the clip range
    l, g, p = out["entropy_coef"]
    assert _same(l, l0) and not _same(g, g0)
    assert _same(g[crit:], g0[crit:])  # the entropy term reaches the actor only
    l, g, p = out["lr_actor"]
    assert _same(l, l0) and _same(g, g0) and _same(p[crit:], p0[crit:]) and not _same(p[:crit], p0[:crit])
    l, g, p = out["lr_critic"]
    assert _same(l, l0) and _same(g, g0) and _same(p[:crit], p0[:crit]) and not _same(p[crit:], p0[crit:])


@pytest.mark.parametrize("Bm", [64, 4096])
def test_phase_split_hyper_calls(Bm):
    """FORWARD, BACKWARD and UPDATE as three uavhip_ppo_step_hyper calls (the data-parallel step's
    shape: k_loss_sums after the forward, k_grad_norm -- the second place Adam's scalars are formed --
    ahead of the update) with OTHER in the buffer:
      * bitwise the three by-value calls on a descriptor holding OTHER;
      * loss sums and raw gradients bitwise those of FORWARD | BACKWARD in one call (k_loss_sums and
        the backward sum the partials in one order);
      * with max_grad_norm far above the norm (the clip coefficient is exactly 1 whichever kernel
        summed g^2, and g * 1 == g), everything bitwise the FULL step's."""
    from uavhip import _lib
    c = _case(Bm, 0)

    def split(tr):
        for b in range(2):
            rows = c.rows(b)
            tr.step(_lib.PPO_FORWARD | tr._packed(b), rows)
            tr.step(_lib.PPO_BACKWARD, rows)
            raw = (tr.loss_sums.clone(), tr.grads.clone())
            tr.step(_lib.PPO_UPDATE, rows)
        return _state(tr), raw

    def hyper(**kw):
        tr = c.trainer(**kw)
        tr.set_hyper(**OTHER)
        return tr

    got, _ = split(hyper())
    want, _ = split(c.trainer(OTHER))
    _assert_same(got, want, "phase-split, buffer vs by value")
    got, raw = split(hyper(max_grad_norm=1e9))
    full = hyper(max_grad_norm=1e9)
    for b in range(2):
        if b == 1:
            full.step(_lib.PPO_FORWARD | _lib.PPO_BACKWARD | full._packed(b), c.rows(b))
            torch.cuda.synchronize()
            assert _same(full.loss_sums, raw[0]) and _same(full.grads, raw[1])
            full.step(_lib.PPO_UPDATE, c.rows(b))
        else:
            full.step(_lib.PPO_FULL, c.rows(b))
    st = _state(full)
    for k in ("params", "adam_m", "adam_v", "adam_step", "grads", "loss_sums"):
        assert _same(got[k], st[k]), f"phase-split vs FULL: {k}"


def test_captured_epoch_follows_the_buffer():
    """One epoch captured after set_hyper, replayed; new values; replayed again: the same graph
    object, and after each replay the parameters of eager by-value epochs with the respective values."""
    from uavhip.policy import TransformerActorCritic
    from uavhip.train import FusedPPOTrainer
    Bm, steps = 64, 4
    torch.manual_seed(51)
    base = TransformerActorCritic().cuda()
    bufs = _buffers(steps * Bm, seed=52)
    A = dict(lr_actor=3e-4, lr_critic=8e-4, entropy_coef=0.02, eps_clip=0.15)
    tr = FusedPPOTrainer(copy.deepcopy(base), Bm)
    tr.set_buffers(*bufs)
    tr.capture()  # a graph of the by-value step: dropped by the first set_hyper
    old = tr.graphs[steps]
    tr.set_hyper(**A)
    assert tr.graphs == {}
    gen = torch.Generator().manual_seed(53)
    s1 = tr.run(epochs=1, generator=gen)
    g1 = tr.graphs[steps]
    assert g1 is not old and list(tr.graphs) == [steps]
    p1 = _state(tr)
    tr.set_hyper(**OTHER)
    assert tr.graphs[steps] is g1
    s2 = tr.run(epochs=1, generator=gen)
    assert tr.graphs[steps] is g1 and list(tr.graphs) == [steps]
    p2 = _state(tr)
    tr.set_hyper(lr_actor=0.0)  # a partial change keeps the others
    assert tr.hyper.tolist() == [0.0, OTHER["lr_critic"], OTHER["entropy_coef"], OTHER["eps_clip"]]

    ref = FusedPPOTrainer(copy.deepcopy(base), Bm, **A)
    ref.set_buffers(*bufs)
    gen = torch.Generator().manual_seed(53)
    r1 = ref.run(epochs=1, generator=gen, use_graph=False)
    q1 = _state(ref)
    for k, v in OTHER.items():
        setattr(ref.desc, k, v)
    r2 = ref.run(epochs=1, generator=gen, use_graph=False)
    q2 = _state(ref)
    assert ref.hyper is None and ref.graphs == {}
    assert s1 == r1 and s2 == r2
    for k in ("params", "adam_m", "adam_v", "adam_step"):
        assert _same(p1[k], q1[k]), f"first replay: {k}"
        assert _same(p2[k], q2[k]), f"replay after set_hyper: {k}"
    assert not _same(p1["params"], p2["params"])


# ------------------------------------------------------------------ the driver
SHAPE = dict(envs=64, uavs=4, targets=4, horizon=16, minibatch=64)
SEED, RESET = 5, 2
SCHED = dict(lr_schedule="linear", lr_final_frac=0.1, entropy_schedule="linear", entropy_final_frac=0.0,
             schedule_iterations=6, lr_warmup=2)
VOLATILE = ("wall_s", "env_steps_per_s")


def make_run(out, **kw):
    from uavhip.fit import TrainingRun
    args = dict(SHAPE, out_dir=str(out), seed=SEED, reset_episodes=RESET, diagnostics_every=0)
    args.update(kw)
    return TrainingRun(**args)


def snapshot(run):
    torch.cuda.synchronize()
    return {k: getattr(run.trainer, k).detach().cpu().clone() for k in ("params", "adam_m", "adam_v", "adam_step")}


def progress(out):
    with open(os.path.join(str(out), "progress.jsonl")) as fh:
        return [json.loads(line) for line in fh]


@pytest.fixture(scope="module")
def scheduled_run(tmp_path_factory):
    """Four iterations with linear lr (warm-up 2) and entropy schedules; fit(2) leaves state_it2.pt."""
    out = tmp_path_factory.mktemp("scheduled")
    run = make_run(out, **SCHED)
    run.fit(2)
    summary = run.fit(4)
    return {"out": out, "at4": snapshot(run), "summary": summary, "graphs": dict(run.trainer.graphs)}


def test_driver_equals_the_hand_written_loop_with_by_value_fields(scheduled_run):
    """The seeding contract of uavhip/fit.py by hand, the descriptor's by-value fields set per
    iteration from schedule_value, eager steps of uavhip_ppo_step: the driver's final parameters."""
    from uavhip import fit
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
    lines = progress(scheduled_run["out"])
    assert [r["iteration"] for r in lines] == [1, 2, 3, 4]
    K, W = SCHED["schedule_iterations"], SCHED["lr_warmup"]
    for i in range(1, 5):
        s_lr = fit.schedule_value("linear", i, K, SCHED["lr_final_frac"], W)
        s_en = fit.schedule_value("linear", i, K, SCHED["entropy_final_frac"])
        want = dict(lr_actor=cfg.LR_ACTOR * s_lr, lr_critic=cfg.LR_CRITIC * s_lr, entropy_coef=0.01 * s_en,
                    eps_clip=cfg.EPS_CLIP * 1.0)
        line = lines[i - 1]
        assert {k: line[k] for k in fit.SCHEDULE_PROGRESS_FIELDS} == want, (i, line)
        assert list(line)[:len(fit.PROGRESS_FIELDS) + 4] == list(fit.PROGRESS_FIELDS + fit.SCHEDULE_PROGRESS_FIELDS)
        for k, v in want.items():
            setattr(trainer.desc, k, v)
        eng.collect()
        trainer.run(epochs=cfg.K_EPOCHS, generator=gen, use_graph=False)
    torch.cuda.synchronize()
    assert trainer.hyper is None
    assert lines[0]["lr_actor"] == cfg.LR_ACTOR * 0.5 and lines[2]["lr_actor"] < lines[1]["lr_actor"]  # ramp, then decay
    assert _same(trainer.params.cpu(), scheduled_run["at4"]["params"])
    assert _same(trainer.adam_m.cpu(), scheduled_run["at4"]["adam_m"])
    assert _same(trainer.adam_step.cpu(), scheduled_run["at4"]["adam_step"])
    # one epoch graph for the whole run, and the summary names the schedules
    assert len(scheduled_run["graphs"]) == 1
    assert scheduled_run["summary"]["schedule"] == dict(fit.SCHEDULE_DEFAULTS, **SCHED)


def test_scheduled_resume_is_exact(scheduled_run, tmp_path):
    state = os.path.join(str(scheduled_run["out"]), "state_it2.pt")
    assert os.path.isfile(state)
    saved = torch.load(state, map_location="cpu", weights_only=True)
    assert saved["hp.lr_schedule"] == "linear" and saved["hp.schedule_iterations"] == 6 and saved["hp.lr_warmup"] == 2
    run = make_run(tmp_path / "resumed", resume=state, **SCHED)
    assert run.iteration == 2
    run.fit(4)
    for k, v in snapshot(run).items():
        assert _same(v, scheduled_run["at4"][k]), k
    a, b = progress(scheduled_run["out"]), progress(tmp_path / "resumed")
    assert [r["iteration"] for r in b] == [3, 4]
    for ra, rb in zip(a[2:], b):
        assert list(ra) == list(rb)
        for k in ra:
            if k not in VOLATILE:
                assert ra[k] == rb[k], (ra["iteration"], k, ra[k], rb[k])
    with pytest.raises(ValueError, match="resume: schedule_iterations differs"):
        make_run(tmp_path / "other", resume=state, **dict(SCHED, schedule_iterations=8))
    with pytest.raises(ValueError, match="resume: lr_schedule differs"):
        make_run(tmp_path / "other", resume=state)


def test_constant_run_is_the_run_without_the_arguments(tmp_path):
    from uavhip import fit
    plain = make_run(tmp_path / "plain")
    s0 = plain.fit(2)
    const = make_run(tmp_path / "const", lr_schedule="constant", entropy_schedule="constant", clip_schedule="constant",
                     lr_final_frac=0.0, entropy_final_frac=0.0, clip_final_frac=1.0, schedule_iterations=0, lr_warmup=0)
    s1 = const.fit(2)
    assert plain.trainer.hyper is None and const.trainer.hyper is None  # set_hyper was never called
    a, b = snapshot(plain), snapshot(const)
    for k in a:
        assert _same(a[k], b[k]), k
    for out in (tmp_path / "plain", tmp_path / "const"):
        for line in progress(out):
            assert list(line) == list(fit.PROGRESS_FIELDS)
    assert "schedule" not in s0 and "schedule" not in s1
    for ra, rb in zip(progress(tmp_path / "plain"), progress(tmp_path / "const")):
        assert {k: v for k, v in ra.items() if k not in VOLATILE} == {k: v for k, v in rb.items() if k not in VOLATILE}


def test_clip_schedule_through_the_driver_reaches_the_step_and_the_diagnostics(tmp_path):
    """clip_schedule="linear" to a quarter over 3 iterations, diagnostics every iteration: each progress
    line carries that iteration's clip range; its clip fractions are update_diagnostics' on the same
    policy and batch with that value (not with the base range, which counts fewer ratios as clipped);
    and the parameters are those of a hand-written loop with the descriptor's eps_clip set per iteration."""
    from uavhip import fit
    from uavhip.config import cfg
    from uavhip.policy import TransformerActorCritic
    from uavhip.ppo import update_diagnostics
    from uavhip.rollout import RolloutEngine
    from uavhip.train import FusedPPOTrainer
    from uavhip.vec_env import VecUAVEnv
    sched = dict(clip_schedule="linear", clip_final_frac=0.25, schedule_iterations=3)
    run = make_run(tmp_path / "clip", diagnostics_every=1, **sched)
    seen = []
    for i in (1, 2, 3):
        line = run.step()
        want = cfg.EPS_CLIP * fit.schedule_value("linear", i, 3, 0.25)
        assert line["eps_clip"] == want and run.used["eps_clip"] == want
        assert line["lr_actor"] == cfg.LR_ACTOR and line["entropy_coef"] == 0.01
        mine = update_diagnostics(run.policy, *run.bufs[:5], eps_clip=want)
        base = update_diagnostics(run.policy, *run.bufs[:5], eps_clip=cfg.EPS_CLIP)
        for k in ("clip_frac", "value_clip_frac", "approx_kl"):
            assert line[k] == float(mine[k]), (i, k, line[k], float(mine[k]))
        seen.append((line["clip_frac"], float(base["clip_frac"]), line["value_clip_frac"], float(base["value_clip_frac"])))
    assert [cfg.EPS_CLIP * x for x in (1.0, 0.625, 0.25)] == [l["eps_clip"] for l in progress(tmp_path / "clip")]
    # a narrower range clips more: the diagnostics did not get the base value
    for clip, clip_base, vclip, vclip_base in seen[1:]:
        assert clip >= clip_base and vclip >= vclip_base and (clip > clip_base or vclip > vclip_base), seen
    got = snapshot(run)

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
    for i in (1, 2, 3):
        trainer.desc.eps_clip = cfg.EPS_CLIP * fit.schedule_value("linear", i, 3, 0.25)
        eng.collect()
        trainer.run(epochs=cfg.K_EPOCHS, generator=gen, use_graph=False)
    torch.cuda.synchronize()
    for k in ("params", "adam_m", "adam_v", "adam_step"):
        assert _same(getattr(trainer, k).cpu(), got[k]), k
