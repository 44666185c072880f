"""The batched training driver: rollout -> episode statistics -> PPO update -> diagnostics ->
evaluation -> progress line -> checkpoints, iteration after iteration, on one GPU.

    run = TrainingRun(envs=4096, uavs=16, targets=32, horizon=64, minibatch=4096, out_dir="runs/a", seed=0)
    run.fit(iterations=200)                      # writes runs/a/final_model.pth, progress.jsonl, state_it200.pt
    TrainingRun(..., out_dir="runs/a", resume="runs/a").fit(iterations=200)   # continues, bit for bit
    TrainingRun(..., out_dir="runs/b", init="runs/clone/final_model.pth")     # starts from a checkpoint (uavhip.imitate)

    python -m uavhip.fit --envs 4096 --uavs 16 --targets 32 --horizon 64 --minibatch 4096 \
        --iterations 200 --out runs/a [--resume runs/a | --init model.pth]   # prints one JSON line at the end

One iteration: RolloutEngine.collect() (a hipGraph replay), EpisodeStats.update(traj),
FusedPPOTrainer.run() over all T * E transitions (the trainer's buffers are views of the engine's
trajectory), update diagnostics (uavhip.ppo.update_diagnostics) every `diagnostics_every`
iterations, a greedy evaluation on fixed scenes against the non-learned baseline every `eval_every`
iterations, one line appended to OUT/progress.jsonl, checkpoints every `checkpoint_every`.

Seeding contract (tests/test_gpu_fit.py rebuilds the loop by hand from it):
    torch.manual_seed(seed) before TransformerActorCritic();
    VecUAVEnv(seed=seed, full_reset_period=reset_episodes or cfg.RESET_EPISODES);
    RolloutEngine(seed=seed), then start();
    minibatch orders from torch.Generator().manual_seed(seed), continuing across iterations.
Capturing the rollout graph runs one warm-up iteration; the driver puts the device state back to
what start() left, so iteration 1 is the iteration an eager collect() after start() would run.

Stop and continue: state_it{K}.pt holds everything iteration K + 1 reads (STATE_TENSORS below and the
hyper-parameters), as one flat dict that torch.load(weights_only=True) reads back. The rollout samples
from counters, the update is deterministic and graph replays equal direct launches, so a resumed run
continues bit for bit. The actor ring (rowproj) is rebuilt by every iteration's first step and is not
saved.

Schedules: lr_schedule / entropy_schedule / clip_schedule ("constant", "linear", "cosine") scale both
learning rates, the entropy coefficient and the clip range by schedule_value(kind, i, K, final_frac)
for iteration i = 1, 2, ... over K = schedule_iterations iterations (held at final_frac from K on);
lr_warmup ramps the learning rates up over the first W iterations. The values are constant within an
iteration and written with FusedPPOTrainer.set_hyper before its update: the step reads them from
device memory (uavhip_ppo_step_hyper), so the captured epoch graph is replayed unchanged. They are a
function of the iteration number alone, so a resumed run continues bit for bit. A run without a
schedule never calls set_hyper and writes the same progress lines as before.

    TrainingRun(..., lr_schedule="linear", lr_final_frac=0.1, lr_warmup=5, schedule_iterations=300)
    python -m uavhip.fit ... --lr-schedule cosine --entropy-schedule linear --schedule-iterations 300

Out of scope: per-minibatch schedules and adaptive (KL-driven) rates, more than one GPU, the
reference's matplotlib curve and its per-episode CSV (uavhip.metrics.csv_rows stays available).
"""
import glob
import json
import math
import os
import re
import time

import torch

from .config import cfg

STATE_FORMAT = "uavhip.fit.state/1"

#: progress.jsonl: the fields of every line, in order; then DIAG_FIELDS when the diagnostics ran and
#: EVAL_FIELDS when the evaluation ran. NaN is written as null.
PROGRESS_FIELDS = ("iteration", "env_steps", "episodes", "mean_ep_reward", "mean_ep_steps", "mean_ep_J",
                   "loss_actor", "loss_critic", "entropy", "epochs_run", "optimizer_steps", "wall_s",
                   "env_steps_per_s")
DIAG_FIELDS = ("approx_kl", "clip_frac", "ratio_max", "ratio_mean", "value_clip_frac", "explained_var", "nonfinite",
               "return_var", "residual_var")
EVAL_FIELDS = ("eval_mean_J", "eval_mean_J_baseline", "eval_beats_baseline")

#: the shape and hyper-parameters a state file records; --resume refuses a state where one differs
HYPER_FIELDS = ("envs", "uavs", "targets", "horizon", "minibatch", "seed", "epochs", "target_kl", "reset_episodes",
                "lr_actor", "lr_critic", "eps_clip", "max_grad_norm", "value_coef", "entropy_coef", "gamma",
                "gae_lambda")

#: the schedule settings, saved as hp.* like HYPER_FIELDS; a state without them was written by an
#: all-constant run (SCHEDULE_DEFAULTS), and --resume refuses a state where one differs
SCHEDULE_FIELDS = ("lr_schedule", "entropy_schedule", "clip_schedule", "lr_final_frac", "entropy_final_frac",
                   "clip_final_frac", "schedule_iterations", "lr_warmup")
SCHEDULE_DEFAULTS = dict(lr_schedule="constant", entropy_schedule="constant", clip_schedule="constant",
                         lr_final_frac=0.0, entropy_final_frac=0.0, clip_final_frac=1.0, schedule_iterations=0,
                         lr_warmup=0)
SCHEDULE_KINDS = ("constant", "linear", "cosine")
#: progress.jsonl: the values the iteration's update used, after PROGRESS_FIELDS, in a scheduled run only
SCHEDULE_PROGRESS_FIELDS = ("lr_actor", "lr_critic", "entropy_coef", "eps_clip")

ENV_TENSORS = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")
KEEP_STATES = 2


def validate_shape(envs, uavs, targets, horizon, minibatch, eval_every=0):
    """The argument checks of TrainingRun that need no device; each message names the argument."""
    if minibatch <= 0 or minibatch % 64:
        raise ValueError(f"minibatch={minibatch}: must be a positive multiple of 64 (the training step's tile)")
    if envs <= 0 or horizon <= 0:
        raise ValueError(f"envs={envs} and horizon={horizon} must be positive")
    if horizon * envs < minibatch:
        raise ValueError(f"minibatch={minibatch} exceeds horizon * envs = {horizon} * {envs} = {horizon * envs}: "
                         "an iteration would run no optimizer step")
    if eval_every > 0 and (uavs > 64 or targets > 64):
        raise ValueError(f"eval_every={eval_every}: the evaluation decodes with N, M <= 64 "
                         f"(uavs={uavs}, targets={targets}); pass eval_every=0")


def schedule_value(kind, i, K, final_frac, warmup=0):
    """The factor a scheduled hyper-parameter is multiplied by in iteration i = 1, 2, ... (Python
    floats): 1 at i = 1, final_frac from i = K on, linear or half-cosine in between; for i <= warmup
    the factor is also multiplied by i / warmup (the learning rates' ramp). "constant": 1 (K unused)."""
    if kind not in SCHEDULE_KINDS:
        raise ValueError(f"schedule kind {kind!r}: must be one of {SCHEDULE_KINDS}")
    if i < 1:
        raise ValueError(f"schedule iteration i={i}: iterations count from 1")
    if kind == "constant":
        s = 1.0
    else:
        if K < 2:
            raise ValueError(f"schedule_iterations={K}: must be >= 2")
        p = min(1.0, (i - 1) / (K - 1))
        shape = 1.0 - p if kind == "linear" else 0.5 * (1.0 + math.cos(math.pi * p))
        s = final_frac + (1.0 - final_frac) * shape
    if i <= warmup:
        s *= i / warmup
    return s


def validate_schedule(sched):
    """The checks of the schedule arguments (a dict of SCHEDULE_FIELDS); each message names the argument."""
    for k in ("lr_schedule", "entropy_schedule", "clip_schedule"):
        if sched[k] not in SCHEDULE_KINDS:
            raise ValueError(f"{k}={sched[k]!r}: must be one of {SCHEDULE_KINDS}")
    for k in ("lr_final_frac", "entropy_final_frac", "clip_final_frac"):
        if not (math.isfinite(sched[k]) and 0.0 <= sched[k] <= 1.0):
            raise ValueError(f"{k}={sched[k]!r}: must lie in [0, 1]")
    if sched["lr_warmup"] < 0:
        raise ValueError(f"lr_warmup={sched['lr_warmup']}: must be >= 0 iterations")
    shaped = any(sched[k] != "constant" for k in ("lr_schedule", "entropy_schedule", "clip_schedule"))
    if shaped and sched["schedule_iterations"] < 2:
        raise ValueError(f"schedule_iterations={sched['schedule_iterations']}: must be >= 2 when a schedule is not "
                         "constant")
    if not shaped and sched["schedule_iterations"] < 0:
        raise ValueError(f"schedule_iterations={sched['schedule_iterations']}: must be >= 0")
    if sched["clip_schedule"] != "constant" and sched["clip_final_frac"] <= 0.0:
        raise ValueError(f"clip_final_frac={sched['clip_final_frac']!r}: the clip range must stay > 0")


def scheduled(sched):
    """Whether any value changes during the run (else the run never calls set_hyper)."""
    return any(sched[k] != "constant" for k in ("lr_schedule", "entropy_schedule", "clip_schedule")) or \
        sched["lr_warmup"] > 0


def schedule_hyper(hyper, sched, i):
    """The four values iteration i's update uses: {lr_actor, lr_critic, entropy_coef, eps_clip}."""
    K = sched["schedule_iterations"]
    s_lr = schedule_value(sched["lr_schedule"], i, K, sched["lr_final_frac"], sched["lr_warmup"])
    s_ent = schedule_value(sched["entropy_schedule"], i, K, sched["entropy_final_frac"])
    s_clip = schedule_value(sched["clip_schedule"], i, K, sched["clip_final_frac"])
    return dict(lr_actor=hyper["lr_actor"] * s_lr, lr_critic=hyper["lr_critic"] * s_lr,
                entropy_coef=hyper["entropy_coef"] * s_ent, eps_clip=hyper["eps_clip"] * s_clip)


def save_state(state, path):
    """One torch.save of a flat dict of tensors / ints / floats / strings (written to a temporary
    name first: a stop in the middle never leaves a truncated state file)."""
    for k, v in state.items():
        if not isinstance(k, str) or not isinstance(v, (torch.Tensor, int, float, str)):
            raise TypeError(f"state[{k!r}]: {type(v).__name__} is not a tensor, int, float or str")
    tmp = path + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, path)


def load_state(path):
    state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict) or state.get("format") != STATE_FORMAT:
        raise ValueError(f"{path}: not a {STATE_FORMAT} training state")
    return state


def latest_state(path):
    """A state file itself, or the state_it{K}.pt with the largest K of a run directory."""
    if os.path.isdir(path):
        found = [(int(m.group(1)), p) for p in glob.glob(os.path.join(path, "state_it*.pt"))
                 for m in [re.search(r"state_it(\d+)\.pt$", p)] if m]
        if not found:
            raise FileNotFoundError(f"{path}: no state_it*.pt to resume from")
        return max(found)[1]
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    return path


def check_compatible(state, hyper):
    """Refuse a state whose shape or hyper-parameters differ from the run's, naming the field."""
    for k in HYPER_FIELDS:
        have, want = state.get("hp." + k), hyper[k]
        if have is None:
            raise ValueError(f"resume: the state has no field {k}")
        same = have == want or (isinstance(have, float) and isinstance(want, float) and
                                math.isnan(have) and math.isnan(want))
        if not same:
            raise ValueError(f"resume: {k} differs: the state was written with {k}={have!r}, this run has "
                             f"{k}={want!r}")
    for k in SCHEDULE_FIELDS:  # absent (a state or a run from before the schedules): all-constant
        have, want = state.get("hp." + k, SCHEDULE_DEFAULTS[k]), hyper.get(k, SCHEDULE_DEFAULTS[k])
        if have != want:
            raise ValueError(f"resume: {k} differs: the state was written with {k}={have!r}, this run has "
                             f"{k}={want!r}")


def _json_value(v):
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return v


def progress_line(fields):
    """One progress.jsonl line: non-finite floats as null."""
    return json.dumps({k: _json_value(v) for k, v in fields.items()})


class TrainingRun:
    def __init__(self, envs, uavs, targets, horizon, minibatch, out_dir, seed=0, epochs=None, target_kl=None,
                 diagnostics_every=1, eval_every=0, eval_scenes=1024, eval_seed=1, checkpoint_every=0,
                 reset_episodes=None, resume=None, lr_actor=None, lr_critic=None, eps_clip=None, max_grad_norm=None,
                 value_coef=0.5, entropy_coef=0.01, device="cuda:0", init=None, lr_schedule="constant",
                 entropy_schedule="constant", clip_schedule="constant", lr_final_frac=0.0, entropy_final_frac=0.0,
                 clip_final_frac=1.0, schedule_iterations=0, lr_warmup=0):
        """target_kl: run the update epoch by epoch and drop the remaining epochs once the
        diagnostics' APPROX_KL exceeds it (None: one run() call of `epochs` epochs).
        resume: a state file, or a run directory (its latest state).
        init: a policy checkpoint (checkpoint.save_checkpoint's format, e.g. uavhip.imitate's
        final_model.pth) loaded into the seeded policy before training starts; everything else is
        seeded as without it. Not with resume (a state carries its own parameters), and not a
        hyper-parameter: state files do not record it.
        lr_schedule / entropy_schedule / clip_schedule, *_final_frac, schedule_iterations, lr_warmup:
        the schedules (module docstring, schedule_value); schedule_iterations is the schedule's own
        length K, whatever number of iterations a fit() call runs."""
        if init is not None and resume is not None:
            raise ValueError("init and resume exclude each other: a resumed state carries its own parameters")
        self.init = None if init is None else str(init)
        self.E, self.N, self.M, self.T = int(envs), int(uavs), int(targets), int(horizon)
        self.minibatch = int(minibatch)
        validate_shape(self.E, self.N, self.M, self.T, self.minibatch, int(eval_every))
        self.epochs = int(cfg.K_EPOCHS if epochs is None else epochs)
        if self.epochs < 1:
            raise ValueError(f"epochs={self.epochs}: must be >= 1")
        for name, v in (("diagnostics_every", diagnostics_every), ("eval_every", eval_every),
                        ("checkpoint_every", checkpoint_every)):
            if int(v) < 0:
                raise ValueError(f"{name}={v}: must be >= 0 (0 = off)")
        self.target_kl = None if target_kl is None else float(target_kl)
        self.diagnostics_every, self.eval_every = int(diagnostics_every), int(eval_every)
        self.eval_scenes, self.eval_seed = int(eval_scenes), int(eval_seed)
        self.checkpoint_every = int(checkpoint_every)
        self.seed = int(seed)
        self.out_dir = str(out_dir)
        self.hyper = dict(
            envs=self.E, uavs=self.N, targets=self.M, horizon=self.T, minibatch=self.minibatch, seed=self.seed,
            epochs=self.epochs, target_kl=float("nan") if self.target_kl is None else self.target_kl,
            reset_episodes=int(cfg.RESET_EPISODES if reset_episodes is None else reset_episodes),
            lr_actor=float(cfg.LR_ACTOR if lr_actor is None else lr_actor),
            lr_critic=float(cfg.LR_CRITIC if lr_critic is None else lr_critic),
            eps_clip=float(cfg.EPS_CLIP if eps_clip is None else eps_clip),
            max_grad_norm=float(cfg.GRAD_NORM_CLIP if max_grad_norm is None else max_grad_norm),
            value_coef=float(value_coef), entropy_coef=float(entropy_coef), gamma=float(cfg.GAMMA),
            gae_lambda=float(cfg.GAE_LAMBDA))
        self.schedule = dict(lr_schedule=str(lr_schedule), entropy_schedule=str(entropy_schedule),
                             clip_schedule=str(clip_schedule), lr_final_frac=float(lr_final_frac),
                             entropy_final_frac=float(entropy_final_frac), clip_final_frac=float(clip_final_frac),
                             schedule_iterations=int(schedule_iterations), lr_warmup=int(lr_warmup))
        validate_schedule(self.schedule)
        self.scheduled = scheduled(self.schedule)
        if self.scheduled:  # the base values the schedules scale go through set_hyper: its checks, up front
            from .train import check_hyper
            check_hyper(**{k: self.hyper[k] for k in SCHEDULE_PROGRESS_FIELDS})
        state = None
        if resume is not None:  # read and checked before anything is built
            self.resumed_from = latest_state(str(resume))
            state = load_state(self.resumed_from)
            check_compatible(state, {**self.hyper, **self.schedule})
        if not torch.cuda.is_available():
            raise RuntimeError("uavhip.fit trains on the GPU (HIP) only")
        self.device = torch.device(device)
        os.makedirs(self.out_dir, exist_ok=True)
        self.iteration = 0
        self.best = float("-inf")
        self.wall_s = 0.0
        self.last = None       # the last progress line's fields
        self.used = {k: self.hyper[k] for k in SCHEDULE_PROGRESS_FIELDS}  # the values of the current iteration's update
        self.phase_ms = {k: 0.0 for k in ("rollout", "update", "diagnostics", "drain", "eval", "files")}
        self._build()
        if state is not None:
            self._load(state)

    # ------------------------------------------------------------------ construction
    def _build(self):
        from . import _lib
        from .metrics import EpisodeStats
        from .policy import TransformerActorCritic
        from .rollout import RolloutEngine
        from .train import FusedPPOTrainer
        from .vec_env import VecUAVEnv
        h, dev = self.hyper, self.device
        torch.cuda.set_device(dev)
        torch.manual_seed(self.seed)
        self.policy = TransformerActorCritic().to(dev)
        if self.init is not None:  # before the trainer takes its flat views of the parameters
            from .checkpoint import load_checkpoint
            load_checkpoint(self.policy, self.init)
        self.env = VecUAVEnv(self.E, self.N, self.M, device=dev, seed=self.seed,
                             full_reset_period=h["reset_episodes"])
        self.engine = RolloutEngine(self.env, self.policy, self.T, seed=self.seed)
        self.engine.start()
        self.stats = EpisodeStats(self.E, device=dev)
        self.trainer = FusedPPOTrainer(self.policy, self.minibatch, lr_actor=h["lr_actor"], lr_critic=h["lr_critic"],
                                       eps_clip=h["eps_clip"], max_grad_norm=h["max_grad_norm"],
                                       value_coef=h["value_coef"], entropy_coef=h["entropy_coef"])
        tr, n = self.engine.traj, self.T * self.E
        self.bufs = (tr.obs[:self.T].reshape(n, 5, 14), tr.actions.reshape(n), tr.logp.reshape(n),
                     tr.values.reshape(n), tr.ret.reshape(n), tr.adv.reshape(n))
        self.trainer.set_buffers(*self.bufs)
        self.generator = torch.Generator().manual_seed(self.seed)
        # the graph capture's warm-up runs one iteration: put the device state back afterwards
        before = {k: v.clone() for k, v in self._device_tensors().items()}
        self.engine.capture()
        for k, v in self._device_tensors().items():
            v.copy_(before[k])
        self.diag_out = torch.zeros(_lib.DIAG_COUNT, dtype=torch.float64, device=dev)
        self.diag_ws = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                        torch.empty(int(_lib.LIB.uavhip_ppo_diagnostics_partials(n)), dtype=torch.float64, device=dev))
        self.solver = None
        self.baseline_J = None
        self._ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def _device_tensors(self):
        """Every device tensor a rollout iteration reads and a later one depends on (name -> tensor)."""
        t = {"engine.counter": self.engine.counter, "engine.obs_T": self.engine.traj.obs[self.T]}
        for k, v in self.env._scene.items():
            t["env.scene." + k] = v
        for k in ENV_TENSORS:
            t["env." + k] = getattr(self.env, k)
        return t

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """The full training state: a flat dict of CPU tensors, ints, floats and strings."""
        s = {"format": STATE_FORMAT, "run.iteration": int(self.iteration), "run.best": float(self.best),
             "run.wall_s": float(self.wall_s), "engine.iteration": int(self.engine.iteration),
             "env.seed": int(self.env.desc.seed), "env.flags": int(self.env.desc.flags)}
        for k, v in {**self.hyper, **self.schedule}.items():
            s["hp." + k] = v
        for k, v in self._device_tensors().items():
            s[k] = v.detach().cpu().clone()
        tr = self.trainer
        for k in ("params", "adam_m", "adam_v", "adam_step"):
            s["trainer." + k] = getattr(tr, k).detach().cpu().clone()
        s["stats.acc"] = self.stats.acc.detach().cpu().clone()
        s["generator.state"] = self.generator.get_state().clone()
        return s

    def _load(self, state):
        """Copy a checked state into the buffers in place (the captured graphs keep their addresses)."""
        with torch.no_grad():
            for k, v in self._device_tensors().items():
                if tuple(state[k].shape) != tuple(v.shape) or state[k].dtype != v.dtype:
                    raise ValueError(f"resume: {k} is {state[k].dtype} {tuple(state[k].shape)} in the state, "
                                     f"{v.dtype} {tuple(v.shape)} here")
                v.copy_(state[k])
            for k in ("params", "adam_m", "adam_v", "adam_step"):
                getattr(self.trainer, k).copy_(state["trainer." + k])
            self.stats.acc.copy_(state["stats.acc"])
        self.policy._packed_key = None  # the parameters changed under the pack's key: repack
        self.env.desc.seed = int(state["env.seed"])
        self.env.desc.flags = int(state["env.flags"])
        self.engine.iteration = int(state["engine.iteration"])
        self.generator.set_state(state["generator.state"])
        self.iteration = int(state["run.iteration"])
        self.best = float(state["run.best"])
        self.wall_s = float(state["run.wall_s"])
        # a run stopped after a progress line but before the next state: drop the lines the resumed run
        # is about to write again
        path = os.path.join(self.out_dir, "progress.jsonl")
        if os.path.isfile(path):
            with open(path) as fh:
                lines = [x for x in fh if x.strip()]
            kept = [x for x in lines if json.loads(x)["iteration"] <= self.iteration]
            if len(kept) != len(lines):
                with open(path + ".tmp", "w") as fh:
                    fh.writelines(kept)
                os.replace(path + ".tmp", path)

    def save_state(self):
        path = os.path.join(self.out_dir, f"state_it{self.iteration}.pt")
        save_state(self.state_dict(), path)
        found = sorted((int(m.group(1)), p) for p in glob.glob(os.path.join(self.out_dir, "state_it*.pt"))
                       for m in [re.search(r"state_it(\d+)\.pt$", p)] if m)
        for _, p in found[:-KEEP_STATES]:
            os.remove(p)
        return path

    def _save_model(self, name):
        from .checkpoint import save_checkpoint
        path = os.path.join(self.out_dir, name)
        save_checkpoint(self.policy, path)
        return path

    # ------------------------------------------------------------------ one iteration
    def _diagnostics(self):
        from .ppo import update_diagnostics
        return update_diagnostics(self.policy, *self.bufs[:5], eps_clip=self.used["eps_clip"], out=self.diag_out,
                                  workspace=self.diag_ws)

    def _update(self):
        """-> (actor loss, critic loss, entropy, epochs run, optimizer steps, diagnostics ran)."""
        if self.target_kl is None:
            la, lc, en, cnt = self.trainer.run(epochs=self.epochs, generator=self.generator)
            return la, lc, en, self.epochs, cnt, False
        from . import _lib
        acc, steps, ran = [0.0, 0.0, 0.0], 0, 0
        for _ in range(self.epochs):
            la, lc, en, cnt = self.trainer.run(epochs=1, generator=self.generator)
            acc = [a + b for a, b in zip(acc, (la, lc, en))]
            steps += cnt
            ran += 1
            kl = float(self._diagnostics()[_lib.DIAG["APPROX_KL"]])
            if kl > self.target_kl:
                break
        return acc[0] / ran, acc[1] / ran, acc[2] / ran, ran, steps, True

    def _evaluate(self):
        from .solve import AllocationSolver
        if self.solver is None:  # its own env, ring and counters: the training stream is not touched
            self.solver = AllocationSolver(self.policy, self.N, self.M, samples=1)
            self.baseline_J = self.solver.baseline(num_scenes=self.eval_scenes, seed=self.eval_seed).J.clone()
        J = self.solver.solve(num_scenes=self.eval_scenes, seed=self.eval_seed).J
        return {"eval_mean_J": float(J.mean()), "eval_mean_J_baseline": float(self.baseline_J.mean()),
                "eval_beats_baseline": float((J > self.baseline_J).double().mean())}

    def step(self):
        """One iteration; returns the progress line's fields (also appended to progress.jsonl)."""
        from . import _lib
        from .metrics import derived
        t0 = time.perf_counter()
        ev = self._ev
        self.iteration += 1
        it = self.iteration
        ev[0].record()
        traj = self.engine.collect()
        self.stats.update(traj)
        ev[1].record()
        if self.scheduled:  # this iteration's values, for all its epochs and minibatches
            self.used = schedule_hyper(self.hyper, self.schedule, it)
            self.trainer.set_hyper(**self.used)
        la, lc, en, epochs_run, steps, diag_fresh = self._update()
        ev[2].record()
        want_diag = self.diagnostics_every > 0 and it % self.diagnostics_every == 0
        if want_diag and not diag_fresh:
            self._diagnostics()
        ev[3].record()
        t1 = time.perf_counter()
        rec = self.stats.drain()  # a host sync: everything above has finished
        self.phase_ms["drain"] += (time.perf_counter() - t1) * 1e3
        self.phase_ms["rollout"] += ev[0].elapsed_time(ev[1])
        self.phase_ms["update"] += ev[1].elapsed_time(ev[2])
        self.phase_ms["diagnostics"] += ev[2].elapsed_time(ev[3])
        d = derived(rec)
        mean = (lambda a: float(a.mean())) if len(rec) else (lambda a: float("nan"))
        f = {"iteration": it, "env_steps": it * self.T * self.E, "episodes": int(len(rec)),
             "mean_ep_reward": mean(d["reward"]), "mean_ep_steps": mean(rec[:, _lib.EP["STEPS"]]),
             "mean_ep_J": mean(d["avg_J"]), "loss_actor": float(la), "loss_critic": float(lc), "entropy": float(en),
             "epochs_run": int(epochs_run), "optimizer_steps": int(steps), "wall_s": 0.0, "env_steps_per_s": 0.0}
        if self.scheduled:
            f.update((k, self.used[k]) for k in SCHEDULE_PROGRESS_FIELDS)
        if want_diag:
            f.update(zip(DIAG_FIELDS, self.diag_out.tolist()))
        score = f["mean_ep_reward"]
        if self.eval_every > 0:
            score = float("nan")
            if it % self.eval_every == 0:
                t1 = time.perf_counter()
                f.update(self._evaluate())
                self.phase_ms["eval"] += (time.perf_counter() - t1) * 1e3
                score = f["eval_mean_J"]
        t1 = time.perf_counter()
        if score > self.best:  # NaN never compares larger
            self.best = score
            self._save_model("best_model.pth")
        dt = time.perf_counter() - t0
        self.wall_s += dt
        f["wall_s"] = self.wall_s
        f["env_steps_per_s"] = self.T * self.E / dt
        with open(os.path.join(self.out_dir, "progress.jsonl"), "a") as fh:
            fh.write(progress_line(f) + "\n")
        if self.checkpoint_every > 0 and it % self.checkpoint_every == 0:
            self._save_model(f"checkpoint_it{it}.pth")
            self.save_state()
        self.phase_ms["files"] += (time.perf_counter() - t1) * 1e3
        self.wall_s += time.perf_counter() - t0 - dt  # the checkpoint writes, after the line's own figure
        self.last = f
        return f

    def fit(self, iterations):
        """Run until `iterations` iterations have been done in total (a resumed run continues its
        count), then write final_model.pth and the state. Returns the summary the command line prints."""
        first = self.iteration
        t0 = time.perf_counter()
        while self.iteration < int(iterations):
            self.step()
        torch.cuda.synchronize(self.device)
        dt = time.perf_counter() - t0
        done = self.iteration - first
        final = self._save_model("final_model.pth")
        if not os.path.exists(os.path.join(self.out_dir, "best_model.pth")):
            self._save_model("best_model.pth")  # no finished episode / evaluation yet: the current weights
        state = self.save_state()
        out = {"out": self.out_dir, "iterations": self.iteration, "iterations_run": done,
               "env_steps": self.iteration * self.T * self.E,
               "env_steps_per_s": done * self.T * self.E / dt if done else 0.0,
               "final_model": final, "best_model": os.path.join(self.out_dir, "best_model.pth"), "state": state,
               "best": _json_value(self.best),
               "phase_ms_per_iteration": {k: v / max(1, done) for k, v in self.phase_ms.items()},
               "last": None if self.last is None else {k: _json_value(v) for k, v in self.last.items()}}
        if self.scheduled:
            out["schedule"] = dict(self.schedule)
        return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Train the allocation policy: batched rollout + fused PPO update")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=cfg.NUM_UAVS)
    ap.add_argument("--targets", type=int, default=cfg.NUM_TARGETS)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--minibatch", type=int, default=4096)
    ap.add_argument("--iterations", type=int, required=True, help="total iterations (a resumed run continues its count)")
    ap.add_argument("--out", required=True, help="run directory")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=None, help=f"update epochs per iteration (default {cfg.K_EPOCHS})")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="stop an iteration's update epochs once the approximate KL exceeds this")
    ap.add_argument("--diagnostics-every", type=int, default=1)
    ap.add_argument("--eval-every", type=int, default=0)
    ap.add_argument("--eval-scenes", type=int, default=1024)
    ap.add_argument("--eval-seed", type=int, default=1)
    ap.add_argument("--checkpoint-every", type=int, default=0)
    ap.add_argument("--reset-episodes", type=int, default=None,
                    help=f"episodes between fresh scenes (default {cfg.RESET_EPISODES})")
    ap.add_argument("--resume", default=None, help="a state_it{K}.pt file, or a run directory (its latest state)")
    ap.add_argument("--init", default=None,
                    help="a policy checkpoint to start from (uavhip.imitate's final_model.pth); not with --resume")
    for name in ("lr", "entropy", "clip"):
        ap.add_argument(f"--{name}-schedule", choices=SCHEDULE_KINDS, default="constant",
                        help=f"how the {dict(lr='learning rates', entropy='entropy coefficient', clip='clip range')[name]} "
                             "change over --schedule-iterations")
        ap.add_argument(f"--{name}-final-frac", type=float, default=SCHEDULE_DEFAULTS[f"{name}_final_frac"],
                        help="the share of the base value the schedule ends at, in [0, 1]")
    ap.add_argument("--schedule-iterations", type=int, default=0,
                    help="the schedules' length K in iterations (>= 2; required with a schedule; not --iterations)")
    ap.add_argument("--lr-warmup", type=int, default=0, help="ramp the learning rates up over this many iterations")
    a = ap.parse_args(argv)
    run = TrainingRun(a.envs, a.uavs, a.targets, a.horizon, a.minibatch, a.out, seed=a.seed, epochs=a.epochs,
                      target_kl=a.target_kl, diagnostics_every=a.diagnostics_every, eval_every=a.eval_every,
                      eval_scenes=a.eval_scenes, eval_seed=a.eval_seed, checkpoint_every=a.checkpoint_every,
                      reset_episodes=a.reset_episodes, resume=a.resume, init=a.init, lr_schedule=a.lr_schedule,
                      entropy_schedule=a.entropy_schedule, clip_schedule=a.clip_schedule,
                      lr_final_frac=a.lr_final_frac, entropy_final_frac=a.entropy_final_frac,
                      clip_final_frac=a.clip_final_frac, schedule_iterations=a.schedule_iterations,
                      lr_warmup=a.lr_warmup)
    print(json.dumps(run.fit(a.iterations)))


if __name__ == "__main__":
    main()
