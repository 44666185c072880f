"""Imitation warm start: clone the non-learned baseline (the best-response search on J) into the
policy, from teacher-forced episodes.

    run = ImitationRun(envs=4096, uavs=16, targets=32, minibatch=4096, out_dir="runs/clone", seed=0)
    run.fit(iterations=20)                       # writes runs/clone/final_model.pth and progress.jsonl
    TrainingRun(..., init="runs/clone/final_model.pth").fit(...)        # PPO from the clone (uavhip.fit)

    python -m uavhip.imitate --envs 4096 --uavs 16 --targets 32 --minibatch 4096 --iterations 20 --out runs/clone
    python -m uavhip.fit ... --init runs/clone/final_model.pth
    python -m uavhip.imitate ... --source dagger --expert-share 0.25 --assign-weight 16

One iteration: fresh on-device scenes, the teacher allocation of every scene
(VecUAVEnv.refine_assignments from the empty assignment: AllocationSolver.baseline's search), ONE
uavhip_teacher_steps launch that walks every env along its teacher allocation and records the window
each action was decided on, the action and the env's reward (teacher_batch), then epochs of the
existing fused PPO step over the valid rows (imitation_update).

The update needs no kernel of its own. With advantage A = 1 and old_logp = the current policy's
log-probability of the teacher's action, the ratio is 1 at the first step, min(r A, clip(r) A) = r,
and its gradient is the gradient of log pi(a*|s): likelihood ascent on the teacher's actions. As the
epochs move the policy, rows whose ratio has left [1 - eps, 1 + eps] upwards stop contributing: the
clip is a trust region per batch. old_values = the current values, so the clipped value loss is the
plain (v - R)^2 at the first step, R the discounted return-to-go of the teacher's episode.

ImitationRun(teacher_exchanges=X) / --teacher-exchanges X (source "teacher" only; 0, the default, is the
path above) takes the teacher allocation from VecUAVEnv.search_assignments(None, max_exchanges=X)
instead: the same search with pairwise exchanges between the sweeps.

Seeding contract (tests/test_gpu_imitate.py relies on it): torch.manual_seed(seed) before
TransformerActorCritic(); iteration i = 1, 2, .. draws its scenes with env.desc.seed = seed + i (as
AllocationSolver._generate_scenes sets it) after zeroing istate; minibatch orders from
torch.Generator().manual_seed(seed), continuing across iterations: torch.randperm(rows) per epoch.
Same seed, same parameters, bit for bit. An ImitationRun cannot be resumed.

source = "expert" | "dagger" (ImitationRun(source=...), --source; "teacher", the path above, is the
default) take the labels from uavhip_expert_steps instead: the state-wise expert's action at every
state an env visits (include/uavhip.h has the rule; followed from a reset it is one best-response
sweep from the empty assignment). "expert": every env follows the expert, the labels are the actions
-- the teacher path with the other label definition. "dagger": iteration 1 runs as "expert"; from
iteration 2 the states are the LEARNER's own -- the scenes are generated as above, then
    env.reset(episode=1, obs_out=obs2[0]); steps.zero_()
    policy.decode_steps(env, obs2, rowproj, 0, True, steps, finished, actions=trace, n_max=N * M,
                        greedy_stride=0, seed=seed + i, offset=0, offset_stride=E)     # sampled
    expert_batch(env, trace, follow)       # env.reset(), then ONE uavhip_expert_steps(trace, follow)
with follow[e] = 1 for e < ceil(expert_share * E) (those envs follow the expert instead of their
trace, so expert episodes stay in every batch), and imitation_update fits the policy to the LABELS
on every valid row, assign_weight on the label-1 rows. Rows are not aggregated across iterations.
obs2, rowproj, steps, finished, trace and follow are the run's own buffers. The decode kernel needs
N, M <= 64, so "dagger" refuses more; "expert" does not. The contract above holds unchanged: the
decode draws from Philox counters keyed by seed + i, nothing from a torch generator, so two runs with
one seed end bitwise equal. progress.jsonl gains, for these two sources, label_agreement (the share
of the learner's rows -- the envs that do not follow -- whose action taken equals the label),
assign_agreement (that share over the learner's label-1 rows; null without such rows, as in
iteration 1 -- the update's own figure, the greedy action after the update on every label-1 row, is
fit_assign_agreement there) and rejected_assigns (assigns the env rejected, all envs).
"""
import json
import os
import time
from dataclasses import dataclass
from typing import Optional

import torch

from .config import cfg

PROGRESS_FIELDS = ("iteration", "rows", "nll_before", "nll_after", "agreement", "teacher_mean_J", "rejected")
SOURCES = ("teacher", "expert", "dagger")
EVAL_FIELDS = ("eval_mean_J", "eval_mean_J_baseline", "eval_beats_baseline")


@dataclass
class TeacherBatch:
    obs: torch.Tensor        # [n_max, E, 5, 14] f32: obs[t] is the window step t's action was decided on
    actions: torch.Tensor    # [n_max, E] int8: the teacher's action, -1 at or past an env's end
    returns: torch.Tensor    # [n_max, E] f32: discounted return-to-go, 0 in held rows
    rows: torch.Tensor       # [rows] int32: flat indices (t * E + e) of the valid rows, ascending
    steps: torch.Tensor      # [E] int32: episode lengths
    J: torch.Tensor          # [E] f64: J of the allocation the env accepted (dstate[J])
    teacher_J: torch.Tensor  # [E] f64: J of the teacher allocation (uavhip_refine_assignments')
    rejected: torch.Tensor   # [E] int32: teacher assigns the env rejected


@torch.no_grad()
def teacher_batch(env, assignment=None, max_sweeps=32, gamma=None, exchanges=0):
    """Reset `env`, walk it along `assignment` ([E, N] int32 target ids or -1; None: the baseline,
    env.refine_assignments(None, max_sweeps=max_sweeps), or with exchanges = X > 0 the search with
    pairwise exchanges, env.search_assignments(None, max_exchanges=X, max_sweeps=max_sweeps)) in one
    uavhip_teacher_steps launch of N * M steps, and return the episodes as a TeacherBatch. returns =
    uavhip.ppo.gae with zero values and lambda = 1: ret_t = r_t + gamma (1 - done_t) ret_{t+1}."""
    from . import _lib
    from .ppo import gae
    env.reset()
    if assignment is None and exchanges > 0:
        assignment, teacher_J, _, _ = env.search_assignments(None, max_exchanges=exchanges, max_sweeps=max_sweeps)
    elif assignment is None:
        assignment, teacher_J, _, _ = env.refine_assignments(None, max_sweeps=max_sweeps)
    else:
        _, teacher_J, _, _ = env.refine_assignments(assignment, max_sweeps=0)
    out = env.teacher_steps(assignment)
    returns, _, _ = gae(out["reward"], out["done"], torch.zeros_like(out["reward"], dtype=torch.float32),
                        gamma=cfg.GAMMA if gamma is None else gamma, lam=1.0, normalize=False)
    rows = torch.nonzero(out["actions"].reshape(-1) >= 0).reshape(-1).to(torch.int32)
    return TeacherBatch(out["obs"], out["actions"], returns, rows, out["steps"],
                        env.dstate[:, _lib.DST["J"]].clone(), teacher_J, out["stats"][:, 0].clone())


@dataclass
class ExpertBatch:
    """uavhip_expert_steps' episodes in TeacherBatch's layout: `actions` are the expert's LABELS
    (what imitation_update fits), `taken` the actions the envs took."""
    obs: torch.Tensor        # [n_max, E, 5, 14] f32: obs[t] is the window step t's action was decided on
    actions: torch.Tensor    # [n_max, E] int8: the expert's label, -1 in held rows
    returns: torch.Tensor    # [n_max, E] f32: discounted return-to-go of the walked episode, 0 in held rows
    rows: torch.Tensor       # [rows] int32: flat indices (t * E + e) of the valid rows, ascending
    steps: torch.Tensor      # [E] int32: episode lengths
    J: torch.Tensor          # [E] f64: J of the allocation the env ended on (dstate[J])
    teacher_J: torch.Tensor  # [E] f64: J of the one-sweep expert's allocation (refine_assignments(None, max_sweeps=1))
    rejected: torch.Tensor   # [E] int32: assigns the env rejected
    taken: torch.Tensor      # [n_max, E] int8: the action taken, -1 in held rows
    margin: torch.Tensor     # [n_max, E] f64: the label's margin, 0 in held rows
    stats: torch.Tensor      # [E, 3] int32: rejected assigns, steps with action != label, trace ended
    follow: Optional[torch.Tensor]  # [E] u8 as passed: the envs that followed the expert (None: all)


@torch.no_grad()
def expert_batch(env, actions=None, follow=None, gamma=None):
    """Reset `env`, walk it along the trace `actions` ([N * M, E] int8; None: every env follows the
    expert; follow [E] u8: the envs that do so anyway) in one uavhip_expert_steps launch of N * M
    steps, and return the episodes with the expert's label of every step as an ExpertBatch. returns
    as teacher_batch's, from the walked episode's rewards."""
    from . import _lib
    from .ppo import gae
    env.reset()
    _, expert_J, _, _ = env.refine_assignments(None, max_sweeps=1)
    out = env.expert_steps(actions, follow, n_max=env.N * env.M)
    returns, _, _ = gae(out["reward"], out["done"], torch.zeros_like(out["reward"], dtype=torch.float32),
                        gamma=cfg.GAMMA if gamma is None else gamma, lam=1.0, normalize=False)
    rows = torch.nonzero(out["labels"].reshape(-1) >= 0).reshape(-1).to(torch.int32)
    return ExpertBatch(out["obs"], out["labels"], returns, rows, out["steps"], env.dstate[:, _lib.DST["J"]].clone(),
                       expert_J, out["stats"][:, 0].clone(), out["actions"], out["margin"], out["stats"], follow)


def learner_agreement(batch):
    """(label_agreement, assign_agreement) of an ExpertBatch over the learner's rows (the envs that
    did not follow the expert): the share of rows whose action taken equals the label, and that share
    over the label-1 rows; NaN without such rows."""
    E = batch.steps.numel()
    learner = torch.zeros(E, dtype=torch.bool, device=batch.steps.device) if batch.follow is None else batch.follow == 0
    rows = (batch.actions >= 0) & learner[None, :]
    hit = (batch.taken == batch.actions)
    q = torch.stack([hit[rows].double().mean(), hit[rows & (batch.actions == 1)].double().mean()]).tolist()
    return q[0], q[1]


def _forward(policy, states, actions):
    """(logp, value, logits) of the teacher's actions on `states`, counter-neutral (offset = 0)."""
    from .ppo import DIAG_FORWARD_CHUNK
    n, dev = states.shape[0], states.device
    logp = torch.empty(n, dtype=torch.float32, device=dev)
    value = torch.empty(n, dtype=torch.float32, device=dev)
    logits = torch.empty(n, 2, dtype=torch.float32, device=dev)
    for b0 in range(0, n, DIAG_FORWARD_CHUNK):
        b1 = min(n, b0 + DIAG_FORWARD_CHUNK)
        policy.fused_forward(states[b0:b1], actions=actions[b0:b1], logp=logp[b0:b1], value=value[b0:b1],
                             logits=logits[b0:b1], offset=0)
    return logp, value, logits


def _fit_quality(logp, logits, actions):
    """(mean negative log-likelihood of the teacher's actions, share of rows whose greedy action
    (l1 > l0, a tie gives 0: the decode's rule) is the teacher's, the same share over the teacher's
    action-1 rows alone -- NaN without one), as 0-dim f64 device tensors."""
    greedy = (logits[:, 1] > logits[:, 0]).to(torch.int8)
    hit = (greedy == actions).double()
    return -logp.double().mean(), hit.mean(), hit[actions == 1].mean()


@torch.no_grad()
def build_batch(policy, batch, assign_weight=1.0, pad_to=1):
    """The update's buffers over the valid rows of `batch`, in row order: (states [n, 5, 14],
    actions [n] int8, old_logp [n], old_values [n], returns [n], advantages [n]) f32, rows, and the
    forward's logits [rows, 2]. old_logp / old_values come from one policy.fused_forward(states,
    actions=teacher); advantages are 1.0, assign_weight on the action-1 rows, not normalised. n is
    rows rounded up to a multiple of pad_to; the rows past `rows` are zeros and no minibatch may
    index them."""
    k = int(batch.rows.numel())
    if k < 1:
        raise ValueError("imitation: the teacher batch has no valid row")
    idx = batch.rows.long()
    states = batch.obs.reshape(-1, cfg.SEQ_LEN, cfg.STATE_DIM)[idx]
    actions = batch.actions.reshape(-1)[idx]
    returns = batch.returns.reshape(-1)[idx]
    logp, value, logits = _forward(policy, states, actions)
    adv = torch.where(actions == 1, float(assign_weight), 1.0).to(torch.float32)
    n = -(-k // int(pad_to)) * int(pad_to)
    bufs = (states, actions, logp, value, returns, adv)
    if n > k:
        bufs = tuple(torch.cat([t, t.new_zeros((n - k,) + tuple(t.shape[1:]))]) for t in bufs)
    return bufs, k, logits


def imitation_update(trainer, policy, batch, epochs, generator, assign_weight=1.0, use_graph=False):
    """`epochs` epochs of the fused PPO step (trainer: a FusedPPOTrainer on `policy`) over the valid
    rows of `batch` as a likelihood fit of the teacher's actions (module docstring). Each epoch draws
    torch.randperm(rows, generator); the last minibatch of an epoch is filled with idx -1 padding
    rows, which add nothing. Returns {"rows", "nll_before", "nll_after", "agreement_before",
    "agreement", "assign_agreement", "optimizer_steps"}: the mean negative log-likelihood of the
    teacher's actions and the share of rows whose greedy action is the teacher's, before and after,
    and that share after over the action-1 rows alone (most rows are skips: a policy that never
    assigns already agrees on their share). Forwards with offset = 0: the policy's sampling counter
    does not move."""
    mb = trainer.global_minibatch
    bufs, k, logits = build_batch(policy, batch, assign_weight, pad_to=mb)
    nll0, agree0, _ = _fit_quality(bufs[2][:k], logits, bufs[1][:k])
    trainer.set_buffers(*bufs)
    n = bufs[0].shape[0]
    pad = torch.full((n - k,), -1, dtype=torch.int32)
    perms = [torch.cat([torch.randperm(k, generator=generator).to(torch.int32), pad]) for _ in range(int(epochs))]
    _, _, _, cnt = trainer.run(perms=perms, use_graph=use_graph)
    logp, _, logits = _forward(policy, bufs[0][:k], bufs[1][:k])
    nll1, agree1, assign1 = _fit_quality(logp, logits, bufs[1][:k])
    q = torch.stack([nll0, nll1, agree0, agree1, assign1]).tolist()
    return {"rows": k, "nll_before": q[0], "nll_after": q[1], "agreement_before": q[2], "agreement": q[3],
            "assign_agreement": q[4], "optimizer_steps": int(cnt)}


def validate_args(envs, uavs, targets, minibatch, epochs, eval_every=0, source="teacher", expert_share=0.25,
                  teacher_exchanges=0):
    """ImitationRun's argument checks that need no device; each message names the argument."""
    if minibatch <= 0 or minibatch % 64:
        raise ValueError(f"minibatch={minibatch}: must be a positive multiple of 64 (the training step's tile)")
    if envs <= 0:
        raise ValueError(f"envs={envs} must be positive")
    if not (1 <= uavs <= 64 and 1 <= targets <= 128):
        raise ValueError(f"uavs={uavs} (1..64) / targets={targets} (1..128) out of range")
    if epochs < 1:
        raise ValueError(f"epochs={epochs}: must be >= 1")
    if eval_every < 0:
        raise ValueError(f"eval_every={eval_every}: must be >= 0 (0 = off)")
    if eval_every > 0 and (uavs > 64 or targets > 64):
        raise ValueError(f"eval_every={eval_every}: the evaluation decodes with N, M <= 64 "
                         f"(uavs={uavs}, targets={targets}); pass eval_every=0")
    if source not in SOURCES:
        raise ValueError(f"source={source!r}: must be one of {', '.join(SOURCES)}")
    if source == "dagger" and (uavs > 64 or targets > 64):
        raise ValueError(f"source='dagger': the learner's trace comes from the decode kernel, which needs N, M <= 64 "
                         f"(uavs={uavs}, targets={targets}); source='expert' has no such limit")
    if not 0.0 <= expert_share <= 1.0:
        raise ValueError(f"expert_share={expert_share}: must be in [0, 1]")
    if teacher_exchanges < 0:
        raise ValueError(f"teacher_exchanges={teacher_exchanges}: must be >= 0 (0 = the plain best-response teacher)")
    if teacher_exchanges > 0 and source != "teacher":
        raise ValueError(f"teacher_exchanges={teacher_exchanges}: source='teacher' only (source={source!r} takes its "
                         f"labels from the state-wise expert)")


class ImitationRun:
    def __init__(self, envs, uavs, targets, minibatch, out_dir, seed=0, epochs=None, eval_every=0, eval_scenes=1024,
                 eval_seed=1, max_sweeps=32, assign_weight=1.0, lr_actor=None, lr_critic=None, eps_clip=None,
                 max_grad_norm=None, value_coef=0.5, entropy_coef=0.01, device="cuda:0", source="teacher",
                 expert_share=0.25, teacher_exchanges=0):
        """source: "teacher" (the baseline's episodes), "expert" (the state-wise expert's own walk) or
        "dagger" (the learner's sampled walk, relabelled by the expert; module docstring).
        expert_share: under "dagger", the share of envs that follow the expert instead.
        teacher_exchanges: under "teacher", X > 0 takes the teacher allocation from the search with at
        most X pairwise exchanges (uavhip_search_assignments) instead of the plain refinement."""
        self.E, self.N, self.M = int(envs), int(uavs), int(targets)
        self.minibatch = int(minibatch)
        self.epochs = int(cfg.K_EPOCHS if epochs is None else epochs)
        self.eval_every = int(eval_every)
        self.source, self.expert_share = source, float(expert_share)
        self.teacher_exchanges = int(teacher_exchanges)
        validate_args(self.E, self.N, self.M, self.minibatch, self.epochs, self.eval_every, self.source,
                      self.expert_share, self.teacher_exchanges)
        self.eval_scenes, self.eval_seed = int(eval_scenes), int(eval_seed)
        self.max_sweeps, self.assign_weight = int(max_sweeps), float(assign_weight)
        self.seed = int(seed)
        self.out_dir = str(out_dir)
        if not torch.cuda.is_available():
            raise RuntimeError("uavhip.imitate trains on the GPU (HIP) only")
        from .policy import TransformerActorCritic
        from .train import FusedPPOTrainer
        from .vec_env import VecUAVEnv
        self.device = dev = torch.device(device)
        os.makedirs(self.out_dir, exist_ok=True)
        torch.cuda.set_device(dev)
        torch.manual_seed(self.seed)
        self.policy = TransformerActorCritic().to(dev)
        self.env = VecUAVEnv(self.E, self.N, self.M, device=dev, seed=self.seed, full_reset_period=0, scene_buffers=1)
        self.trainer = FusedPPOTrainer(self.policy, self.minibatch, lr_actor=lr_actor, lr_critic=lr_critic,
                                       eps_clip=eps_clip, max_grad_norm=max_grad_norm, value_coef=value_coef,
                                       entropy_coef=entropy_coef)
        self.generator = torch.Generator().manual_seed(self.seed)
        self.iteration = 0
        self.wall_s = 0.0
        self.last = None
        self.solver = None
        self.baseline_J = None
        self.batch = None  # "expert" / "dagger": the last iteration's ExpertBatch
        self.trace = None  # "dagger": the decode buffers, made at iteration 2

    def _evaluate(self):
        from .solve import AllocationSolver
        if self.solver is None:
            self.solver = AllocationSolver(self.policy, self.N, self.M, samples=1)
            self.baseline_J = self.solver.baseline(num_scenes=self.eval_scenes, seed=self.eval_seed).J.clone()
        J = self.solver.solve(num_scenes=self.eval_scenes, seed=self.eval_seed).J
        return {"eval_mean_J": float(J.mean()), "eval_mean_J_baseline": float(self.baseline_J.mean()),
                "eval_beats_baseline": float((J > self.baseline_J).double().mean())}

    @torch.no_grad()
    def learner_trace(self):
        """The learner's sampled walk over the env's current scenes (module docstring): (trace
        [N * M, E] int8, -1 past an env's end; follow [E] u8). The env is left at the walk's end."""
        import math

        from . import _lib
        from .policy import rowproj_buffer
        env, E, dev = self.env, self.E, self.device
        if self.trace is None:
            self.obs2 = torch.zeros(2, E, _lib.SEQ_LEN, _lib.STATE_DIM, dtype=torch.float32, device=dev)
            self.rowproj = rowproj_buffer(E, dev)
            self.steps = torch.zeros(E, dtype=torch.int32, device=dev)
            self.finished = torch.zeros(E, dtype=torch.uint8, device=dev)
            self.trace = torch.empty(self.N * self.M, E, dtype=torch.int8, device=dev)
            self.follow = torch.zeros(E, dtype=torch.uint8, device=dev)
            self.follow[:math.ceil(self.expert_share * E)] = 1
        env.reset(episode=1, obs_out=self.obs2[0])
        self.steps.zero_()
        self.policy.packed_weights()
        self.policy.decode_steps(env, self.obs2, self.rowproj, 0, True, self.steps, self.finished, actions=self.trace,
                                 n_max=self.N * self.M, greedy_stride=0,
                                 seed=(self.seed + self.iteration) & (2 ** 64 - 1), offset=0, offset_stride=E)
        return self.trace, self.follow

    def step(self):
        """One iteration; returns the progress line's fields (also appended to progress.jsonl)."""
        from .fit import progress_line
        t0 = time.perf_counter()
        self.iteration += 1
        it, env = self.iteration, self.env
        env.desc.seed = (self.seed + it) & (2 ** 64 - 1)
        env.istate.zero_()
        env.generate_scenes()
        if self.source == "teacher":
            batch = teacher_batch(env, None, max_sweeps=self.max_sweeps, exchanges=self.teacher_exchanges)
        else:
            self.batch = None  # run.batch is the last ExpertBatch; released before the next is made
            learner = self.source == "dagger" and it >= 2
            self.batch = batch = expert_batch(env, *(self.learner_trace() if learner else ()))
        q = imitation_update(self.trainer, self.policy, batch, self.epochs, self.generator, self.assign_weight)
        f = {"iteration": it, "rows": q["rows"], "nll_before": q["nll_before"], "nll_after": q["nll_after"],
             "agreement": q["agreement"], "teacher_mean_J": float(batch.teacher_J.mean()),
             "rejected": int(batch.rejected.sum()), "agreement_before": q["agreement_before"],
             "assign_agreement": q["assign_agreement"], "assign_share": float((batch.actions == 1).sum()) / q["rows"],
             "walked_mean_J": float(batch.J.mean()), "optimizer_steps": q["optimizer_steps"]}
        if self.source != "teacher":
            f["label_agreement"], f["assign_agreement"] = learner_agreement(batch)
            f.update(fit_assign_agreement=q["assign_agreement"], rejected_assigns=int(batch.rejected.sum()),
                     trace_ended=int(batch.stats[:, 2].sum()), source=self.source)
        if self.eval_every > 0 and it % self.eval_every == 0:
            f.update(self._evaluate())
        self.wall_s += time.perf_counter() - t0
        f["wall_s"] = self.wall_s
        with open(os.path.join(self.out_dir, "progress.jsonl"), "a") as fh:
            fh.write(progress_line(f) + "\n")
        self.last = f
        return f

    def fit(self, iterations):
        """Run `iterations` iterations in total, then write final_model.pth (the reference's
        checkpoint format: uavhip.solve and uavhip.fit --init load it). Returns the summary the
        command line prints."""
        from .checkpoint import save_checkpoint
        from .fit import _json_value
        while self.iteration < int(iterations):
            self.step()
        torch.cuda.synchronize(self.device)
        final = os.path.join(self.out_dir, "final_model.pth")
        save_checkpoint(self.policy, final)
        return {"out": self.out_dir, "iterations": self.iteration, "final_model": final, "wall_s": self.wall_s,
                "last": None if self.last is None else {k: _json_value(v) for k, v in self.last.items()}}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Clone the best-response baseline into the policy (imitation warm start)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=cfg.NUM_UAVS)
    ap.add_argument("--targets", type=int, default=cfg.NUM_TARGETS)
    ap.add_argument("--minibatch", type=int, default=4096)
    ap.add_argument("--iterations", type=int, required=True)
    ap.add_argument("--out", required=True, help="run directory")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=None, help=f"update epochs per iteration (default {cfg.K_EPOCHS})")
    ap.add_argument("--assign-weight", type=float, default=1.0, help="advantage of the action-1 (assign) rows")
    ap.add_argument("--max-sweeps", type=int, default=32, help="sweeps of the teacher's best-response search")
    ap.add_argument("--eval-every", type=int, default=0)
    ap.add_argument("--eval-scenes", type=int, default=1024)
    ap.add_argument("--eval-seed", type=int, default=1)
    ap.add_argument("--source", choices=SOURCES, default="teacher",
                    help="teacher: the baseline's episodes; expert: the state-wise expert's own walk; dagger: the "
                         "learner's sampled walk relabelled by the expert")
    ap.add_argument("--expert-share", type=float, default=0.25,
                    help="dagger: the share of envs that follow the expert instead of the learner's trace")
    ap.add_argument("--teacher-exchanges", type=int, default=0, metavar="X",
                    help="teacher: the teacher allocation from the search with at most X pairwise exchanges "
                         "(0: the plain best-response search)")
    a = ap.parse_args(argv)
    run = ImitationRun(a.envs, a.uavs, a.targets, a.minibatch, a.out, seed=a.seed, epochs=a.epochs,
                       eval_every=a.eval_every, eval_scenes=a.eval_scenes, eval_seed=a.eval_seed,
                       max_sweeps=a.max_sweeps, assign_weight=a.assign_weight, source=a.source,
                       expert_share=a.expert_share, teacher_exchanges=a.teacher_exchanges)
    print(json.dumps(run.fit(a.iterations)))


if __name__ == "__main__":
    main()
