"""Batched allocation inference: a trained policy and a set of scenes in, allocations out.

The reference's only inference tool is test_visualize.py: one scene, one sampled episode, on the
CPU (policy.get_action -> env.step until done, then the UAVs' assigned_target_id and J). Here every
scene is decoded on the GPU by uavhip_decode_steps -- the ACTOR trunk and head, an action and the
env step per step, nothing else, every env until its own episode ends -- and, with samples = K > 1,
K times: replica 0 of each scene greedily (argmax), the others by sampling, and
uavhip_select_best keeps the replica with the largest objective J(X) (best-of-K, the usual way a
learned constructive solver is used).

    solver = AllocationSolver(policy, num_uavs=16, num_targets=32, samples=8)
    alloc = solver.solve(num_scenes=4096, seed=0)       # or solve(scenes=[scene dicts])
    alloc.assignment[s]   # [N] target id of each UAV (-1: none), alloc.J[s], alloc.covered[s]

    alloc = solver.solve(num_scenes=4096, seed=0, refine=32)   # + best-response local search on J
    base = solver.baseline(num_scenes=4096, seed=0)            # the same scenes without the policy
    alloc = solver.solve(num_scenes=4096, seed=0, refine=32, exchanges=32)   # + pairwise exchanges

The env accepts or rejects an assignment on r(X), in one pass of the pointer walk; refine = R > 0
polishes the chosen replica's allocation on J(X) itself (uavhip_refine_assignments: every UAV in turn
moves to the target, or to none, where its marginal contribution to J is largest, at most R sweeps),
and baseline() runs that search from the empty assignment -- the non-learned yardstick a
checkpoint's mean J is read against. exchanges = X > 0 (solve and baseline) runs the search with a second
neighbourhood instead (uavhip_search_assignments): where no single move improves J, the best swap of
two UAVs' targets is made and the sweeps run again, at most X times. constraints = Constraints(...)
(solve and baseline) runs that search under pairs that may not be flown, UAVs that are already committed
and a limit on the UAVs of one target (uavhip_search_assignments_constrained); the decode ignores them.
optimum() (N <= 16) is the yardstick's yardstick: the largest J any allocation of the scene reaches, by
a subset DP over the UAVs (uavhip_solve_exact), under the same constraints when given.
restarts = R > 0 (solve and baseline) runs the constrained search R times per scene in one launch
(uavhip_search_multistart): replica 0 is what the call does without it, the others start from random
full assignments, and the best J wins -- a near-optimal allocator at every size, constraints included.
solve(restarts=R, starts="replicas") starts that search from ALL K decoded replicas of a scene instead of
the chosen one (uavhip_search_multistart_from): replicas 0..K-1 of the search run from the K allocations
the decode left, the other R - K from random full assignments; refine_stats[:, 8] < K says a policy start
won, and Allocation.start_J holds every replica's J.
lns_rounds = L > 0 (solve and baseline) runs a large-neighbourhood search after whatever search the call
already does, under the same constraints (VecUAVEnv.lns_assignments): L times, lns_free = K <= 16 UAVs of
the scene are freed and re-placed at the optimum of J over all their (M + 1)^K placements
(uavhip_solve_exact_free, at every N <= 64), the others held, and a scene keeps the new allocation only
where its J is strictly larger. Allocation.lns_J_before holds the J going in.

Command line: python -m uavhip.solve --checkpoint PATH --scenes S --samples K [--seed SEED]
[--refine SWEEPS] [--exchanges X] [--baseline] [--optimum] [--restarts R] [--starts replicas]
[--lns ROUNDS --lns-free K --lns-mode {random,targets}] prints one JSON line (mean / best J, mean covered, mean steps,
scenes/s; with the flags also mean_J_decoded / mean_J_refined / mean_J_baseline and the share of
scenes where the policy beats the baseline; with --exchanges also mean_exchanges and, beside the plain
mean_J_baseline, mean_J_baseline_exchange; with --optimum, which implies --baseline, also mean_J_optimal, each
mean J's share of it (baseline_over_optimal, decoded_over_optimal, ...) and the share of scenes where the
baseline reaches it, baseline_is_optimal; with --restarts R also mean_J_multistart, the baseline with R
restarts and --exchanges' cap (32 when that is 0), and with --optimum multistart_over_optimal and
multistart_is_optimal; with --starts replicas, which needs --restarts R >= --samples K >= 2, also
mean_J_policy_starts -- solve(restarts=R, starts="replicas") at --refine's and --exchanges' caps, 32 where
they are 0 --, policy_start_wins, the share of scenes where one of the K policy starts is the chosen replica
(a tie goes to the lowest replica, so to a policy start: read it beside the next key),
policy_starts_beat_random, the share where its J is strictly above mean_J_multistart's scene at the same R,
and with --optimum policy_starts_over_optimal and policy_starts_is_optimal; with --lns ROUNDS, which implies
--baseline, also mean_J_lns -- the baseline with --exchanges' cap, 32 when that is 0, then ROUNDS rounds of
the large-neighbourhood search with --lns-free UAVs free --, lns_improved, the share of scenes it strictly
improved, and with --optimum lns_over_optimal and lns_is_optimal).

The solver owns its env, ring buffer and sampling counters: a training RolloutEngine on the same
policy is not touched (the packed weights are shared through policy.packed_weights()).
"""
from dataclasses import dataclass, fields, replace
from typing import Optional

import numpy as np
import torch

from . import _lib
from .assign import _check_free, _check_mode
from .config import cfg as default_cfg
from .policy import rowproj_buffer
from .vec_env import SCENE_KEYS_F64, VecUAVEnv

RTOL = 1e-12  # the project's bar on J: two J within RTOL max(1, |J|) are the same allocation's up to rounding


@dataclass
class Allocation:
    """Result of AllocationSolver.solve (device tensors; .cpu() moves them to the host)."""
    assignment: torch.Tensor    # [S, N] int32: the target id each UAV locked, -1 for none
    J: torch.Tensor             # [S] f64: objective J(X) of the chosen replica (0 when none finished)
    covered: torch.Tensor       # [S] int32: targets with at least one lock
    best_replica: torch.Tensor  # [S] int32: index of the chosen replica, -1 when none finished
    steps: torch.Tensor         # [S] int32: decode steps of the chosen replica
    replica_J: torch.Tensor     # [S, K] f64: J of every replica as decoding left it
    actions: Optional[torch.Tensor] = None  # [max_steps, S * K] int8 action trace (trace=True)
    start_J: Optional[torch.Tensor] = None  # [S, R] f64: J of every replica of the search (starts="replicas")
    lns_J_before: Optional[torch.Tensor] = None  # [S] f64: J going into the large-neighbourhood search (lns_rounds > 0)
    decoded_J: Optional[torch.Tensor] = None     # [S] f64: J before refinement (solve(refine > 0))
    refine_stats: Optional[torch.Tensor] = None  # [S, 4] int32: sweeps, moves, converged, invalid ids;
    #                                              [S, 6] with exchanges > 0: + exchanges made, scan clean;
    #                                              [S, 8] with constraints: + pairs dropped, fixed conflicts
    #                                              [S, 10] with restarts > 0: + the chosen replica, replicas above replica 0

    def cpu(self):
        return Allocation(*(None if t is None else t.cpu() for t in (getattr(self, f.name) for f in fields(self))))


@dataclass
class Constraints:
    """What solve(constraints=) / baseline(constraints=) hold the local search to, per scene s and in
    the scene's LIST order of targets (as p_dmg's columns); None for "no such constraint". Tensors (or
    arrays) of exactly these dtypes and shapes; they are moved to the solver's device."""
    allowed: Optional[torch.Tensor] = None    # [S, N, M] uint8 / bool: nonzero = UAV u may take target t
    capacity: Optional[torch.Tensor] = None   # [S, M] int32: the most UAVs on target t (< 0 counts as 0)
    fixed_ids: Optional[torch.Tensor] = None  # [S, N] int32: -2 = free, -1 = fixed to none, else the target ID
    #                                           (tgt_id) UAV u is committed to

    def on(self, what, S, N, M, device):
        """Checked against S scenes of N x M, before any device call; then on `device`:
        (allowed uint8, capacity, fixed_ids) with None kept."""
        out = []
        for name, dtypes, shape in (("allowed", (torch.uint8, torch.bool), (S, N, M)),
                                    ("capacity", (torch.int32,), (S, M)), ("fixed_ids", (torch.int32,), (S, N))):
            t = getattr(self, name)
            if t is not None:
                t = torch.as_tensor(t)
                if t.dtype not in dtypes or tuple(t.shape) != shape:
                    raise ValueError(f"{what}: constraints.{name}: need {' or '.join(map(str, dtypes))} {shape} "
                                     f"(got {t.dtype} {tuple(t.shape)})")
            out.append(t)
        return tuple(None if t is None else t.to(device=device, dtype=torch.uint8 if t.dtype == torch.bool else t.dtype)
                     .contiguous() for t in out)


def _check_lns(what, rounds, free, mode):
    """The lns_* arguments of solve / baseline, before any device call."""
    if rounds < 0:
        raise ValueError(f"{what}: lns_rounds must be >= 0")
    if rounds > 0:
        _check_free(what, "lns_free", free)
        _check_mode(what, mode, "lns_mode")


def _with_fixed(assignment, fixed_ids, shape, device):
    """(the start with the committed UAVs' ids written in, the fixed flags) of the constrained search."""
    if fixed_ids is None:
        return assignment, None
    if assignment is None:
        assignment = torch.full(shape, -1, dtype=torch.int32, device=device)
    ids = fixed_ids if assignment.dim() == 2 else fixed_ids[:, None]  # [S, K, N] starts: over every one of the K
    return torch.where(ids != -2, ids, assignment), (fixed_ids != -2).to(torch.uint8)


class AllocationSolver:
    def __init__(self, policy, num_uavs, num_targets, num_nfz=None, num_interceptors=None, config=None, samples=1,
                 device=None):
        p0 = next(policy.parameters())
        if p0.device.type != "cuda":
            raise RuntimeError("AllocationSolver decodes on the GPU (HIP) only: move the policy to a cuda device")
        self.policy = policy
        self.device = torch.device(p0.device if device is None else device)
        if self.device.type != "cuda":
            raise RuntimeError("AllocationSolver decodes on the GPU (HIP) only")
        self.cfg = config or default_cfg
        self.N, self.M = int(num_uavs), int(num_targets)
        if self.N > 64 or self.M > 64:
            raise ValueError(f"the decode kernel needs N, M <= 64 (got {self.N}, {self.M})")
        self.Kn, self.Ki = num_nfz, num_interceptors
        self.K = int(samples)
        if self.K < 1:
            raise ValueError("samples must be >= 1")
        self.env = None

    def _size(self, S):
        """The env of S * K replicas and the decode buffers (kept while S stays the same)."""
        E = S * self.K
        if self.env is None or self.env.E != E:
            dev = self.device
            self.env = VecUAVEnv(E, self.N, self.M, self.Kn, self.Ki, config=self.cfg, device=dev,
                                 full_reset_period=0, scene_buffers=1)
            self.obs2 = torch.zeros(2, E, _lib.SEQ_LEN, _lib.STATE_DIM, dtype=torch.float32, device=dev)
            self.rowproj = rowproj_buffer(E, dev)
            self.steps = torch.zeros(E, dtype=torch.int32, device=dev)
            self.finished = torch.zeros(E, dtype=torch.uint8, device=dev)
            self.ep_return = torch.zeros(E, dtype=torch.float64, device=dev)
        return self.env

    def _load_host_scenes(self, env, scenes):
        """VecUAVEnv.load_scenes for K replicas of each scene: the S scenes go up once, every scene
        array is repeated K times scene-major (e = s * K + k), and the pair tables are scored once."""
        S, K = len(scenes), self.K
        if any(np.size(s["tgt_value"]) and float(np.min(s["tgt_value"])) < 0 for s in scenes):
            env.desc.flags |= _lib.ENV_NO_REPLAY
        sc = env._scene
        for k in SCENE_KEYS_F64 + ("tgt_id", "uav_type"):
            dst = sc[k]
            if k == "uav_type" and not all("uav_type" in s for s in scenes):
                continue
            dt = np.int32 if dst.dtype == torch.int32 else np.float64
            host = np.stack([np.asarray(s[k], dt).reshape(tuple(dst.shape[1:])) if np.size(s[k])
                             else np.zeros(tuple(dst.shape[1:]), dt) for s in scenes])
            dst.copy_(torch.from_numpy(host).to(env.device).repeat_interleave(K, dim=0))
        env.istate.zero_()
        env.score_pairs()
        return S

    def _generate_scenes(self, env, S, seed):
        """S on-device Philox scenes (scene s = the generator's scene of env s under `seed`), each
        with its pair tables repeated K times scene-major."""
        K = self.K
        env.desc.seed = int(seed) & (2 ** 64 - 1)
        env.istate.zero_()
        mask = torch.zeros(env.E, dtype=torch.uint8, device=env.device)
        mask[:S] = 1
        env.generate_scenes(mask)
        if K > 1:
            for t in env._scene.values():
                t.copy_(t[:S].repeat_interleave(K, dim=0))
        env.istate.zero_()

    def _scene_env(self, scenes, S, seed):
        """The env of S * K replicas with the scenes in place (the solver's device current)."""
        env = self._size(S)
        if scenes is not None:
            self._load_host_scenes(env, scenes)
        else:
            self._generate_scenes(env, S, seed)
        return env

    def _prepare(self, what, scenes, num_scenes, seed, constraints, refusals=()):
        """The arguments solve / baseline / optimum (`what`) share, checked before anything is allocated; the caller's
        own (refused, message) pairs come between the constraints' type and the scene arguments. -> (scenes list or
        None, S, seed, limits: (allowed, capacity, fixed_ids) on the solver's device, None without constraints)."""
        if constraints is not None and not isinstance(constraints, Constraints):
            raise ValueError(f"{what}: constraints must be a uavhip.solve.Constraints (got {type(constraints).__name__})")
        for refused, message in refusals:
            if refused:
                raise ValueError(message)
        if (scenes is None) == (num_scenes is None):
            raise ValueError(f"{what}: pass scenes or num_scenes")
        if isinstance(scenes, dict):
            scenes = [scenes]
        S = len(scenes) if scenes is not None else int(num_scenes)
        if S <= 0:
            raise ValueError(f"{what}: no scenes")
        limits = None if constraints is None else constraints.on(what, S, self.N, self.M, self.device)
        return scenes, S, 0 if seed is None else int(seed), limits

    def _undecoded(self, env, S, assignment, J, covered, stats):
        """The Allocation of baseline / optimum: the decode-only fields (best_replica, steps, replica_J) zeros."""
        zi = torch.zeros(S, dtype=torch.int32, device=env.device)
        return Allocation(assignment, J, covered, zi, zi.clone(),
                          torch.zeros(S, self.K, dtype=torch.float64, device=env.device), refine_stats=stats)

    def _decode(self, env, S, seed, max_steps, trace):
        """The scenes in `env` decoded, K replicas each, and the best replica chosen: solve(refine=0)'s Allocation."""
        K = self.K
        n_max = int(self.N * self.M if max_steps is None else max_steps)
        actions = torch.empty(n_max, env.E, dtype=torch.int8, device=env.device) if trace else None
        self.steps.zero_()
        self.ep_return.zero_()
        env.reset(episode=1, obs_out=self.obs2[0])
        self.policy.packed_weights()
        self.policy.decode_steps(env, self.obs2, self.rowproj, 0, True, self.steps, self.finished, actions=actions,
                                 ep_return=self.ep_return, n_max=n_max, greedy_stride=K, seed=seed, offset=0,
                                 offset_stride=env.E)
        best, J, covered, assignment = env.select_best(K)
        replica_J = env.dstate[:, _lib.DST["J"]].reshape(S, K).clone()
        steps = torch.gather(self.steps.view(S, K), 1, best.clamp(min=0).long().view(S, 1)).view(S)
        return Allocation(assignment, J, covered, best, steps, replica_J, actions)

    def _search(self, env, start, S, sweeps, exchanges, restarts, seed, limits):
        """The one search solve / baseline launch on S scenes from `start` [S, N] (None: the empty
        assignment): the multi-start with restarts > 0, else the constrained search under `limits`, else
        the exchange search with exchanges > 0, else the plain refinement. The first two lay the committed
        UAVs' ids over the start. -> (assignment, J, covered, stats)."""
        rows = dict(stride=self.K, rows=S, max_sweeps=sweeps)
        if restarts == 0 and limits is None:
            if exchanges > 0:
                return env.search_assignments(start, max_exchanges=exchanges, **rows)
            return env.refine_assignments(start, **rows)
        allowed, capacity, fixed_ids = limits or (None, None, None)
        start, fixed = _with_fixed(start, fixed_ids, (S, self.N), env.device)
        if restarts > 0:
            return env.search_assignments_multistart(start, allowed, fixed, capacity, restarts=restarts,
                                                     seed=seed & (2 ** 64 - 1), max_exchanges=exchanges, **rows)
        return env.search_assignments_constrained(start, allowed, fixed, capacity, max_exchanges=exchanges, **rows)

    def _lns(self, env, alloc, S, seed, rounds, free, mode, limits):
        """`alloc` after `rounds` rounds of the large-neighbourhood search from its assignment, the
        committed UAVs held; alloc itself when rounds == 0."""
        if rounds == 0:
            return alloc
        allowed, capacity, fixed_ids = limits or (None, None, None)
        fixed = None if fixed_ids is None else (fixed_ids != -2).to(torch.uint8)
        assignment, J, covered, _ = env.lns_assignments(alloc.assignment, rounds=rounds, free=free, mode=mode,
                                                        seed=seed & (2 ** 64 - 1), allowed=allowed, fixed=fixed,
                                                        capacity=capacity, stride=self.K, rows=S)
        return replace(alloc, assignment=assignment, J=J, covered=covered, lns_J_before=alloc.J)

    @torch.no_grad()
    def solve(self, scenes=None, num_scenes=None, seed=None, max_steps=None, trace=False, refine=0, exchanges=0,
              constraints=None, restarts=0, starts="best", lns_rounds=0, lns_free=12, lns_mode="targets"):
        """Decode `scenes` (host scene dicts in the tests/golden / scene.generate_scene layout) or
        `num_scenes` on-device scenes drawn with `seed`; K = samples replicas each (replica 0
        greedy, the rest sampled with Philox key `seed`), at most max_steps steps (default N * M,
        the longest possible episode). Returns an Allocation.
        refine = R > 0: the chosen replica's assignment is polished by at most R sweeps of the
        best-response local search on J (uavhip_refine_assignments); assignment / J / covered are
        then the refined ones, decoded_J the J before and refine_stats the search's counters. A
        scene where no replica finished (best_replica == -1) is refined from the empty assignment.
        refine = 0 launches nothing more and changes nothing.
        exchanges = X > 0 (needs refine > 0): the polish is uavhip_search_assignments with at most X
        pairwise exchanges and R sweeps per phase, refine_stats its [S, 6] counters. exchanges = 0 is
        the plain refinement: the same launches, the same results.
        constraints = Constraints(allowed, capacity, fixed_ids) (needs refine > 0): the DECODE IGNORES
        THEM -- the policy walks the scene as ever. The solver then overwrites the decoded assignment of
        every committed UAV (fixed_ids != -2) with its fixed id and polishes with
        uavhip_search_assignments_constrained (at most X exchanges, X = 0 included), which drops what the
        constraints do not admit and searches within them; refine_stats is its [S, 8] counters and
        decoded_J stays the unconstrained decode's J. constraints = None changes no launch and no result.
        restarts = R > 0 (needs refine > 0): the polish is uavhip_search_multistart with R replicas --
        replica 0 the polish this call would run without it (at most X exchanges, X = 0 included, under
        the constraints when given), replicas 1..R-1 the same search from random full assignments drawn
        with Philox key `seed` -- and the replica with the largest J is kept; refine_stats is [S, 10]: the
        chosen replica's eight counters, its index, the replicas above replica 0. restarts = 0 launches
        nothing new and changes no result.
        starts = "replicas" (needs refine > 0, samples K >= 2 and restarts R >= K; "best", the default, is
        everything above, bitwise): the search starts from ALL K decoded replicas of a scene, not only
        the chosen one (uavhip_search_multistart_from with R0 = K). Replica k < K of the search runs from
        what replica k of the decode assigned -- env.assigned_target_ids() as [S, K, N], an unfinished
        replica included with what it assigned so far --, replicas K..R-1 from random full assignments
        drawn with Philox key `seed`; with constraints the committed UAVs' fixed ids are laid over every
        one of the K starts. decoded_J, best_replica and replica_J stay select_best's; refine_stats[:, 8]
        is the chosen replica r* of the search (r* < K: a policy start won) and start_J [S, R] every
        replica's J. The start of the call with restarts = 0 is one of the K (replica best_replica), its
        search is that replica's bit for bit, so per scene J >= that call's J wherever a replica finished.
        lns_rounds = L > 0: after all of the above, L rounds of VecUAVEnv.lns_assignments from the call's
        assignment -- lns_free UAVs (1..16) freed per round by rule lns_mode ("targets" or "random", Philox
        key `seed`) and re-placed at the optimum of their neighbourhood, under the constraints when given,
        the committed UAVs held. assignment / J / covered are then the search's, lns_J_before the J going
        in; J >= lns_J_before in every scene. lns_rounds = 0 launches nothing more and changes nothing."""
        lns_rounds, lns_free = int(lns_rounds), int(lns_free)
        _check_lns("solve", lns_rounds, lns_free, lns_mode)
        if starts not in ("best", "replicas"):
            raise ValueError(f"solve: starts must be 'best' or 'replicas' (got {starts!r})")
        refine, exchanges, restarts = int(refine), int(exchanges), int(restarts)
        if not 0 <= restarts <= _lib.MULTISTART_MAX_R:
            raise ValueError(f"solve: restarts must be in [0, {_lib.MULTISTART_MAX_R}]")
        if restarts > 0 and refine == 0:
            raise ValueError("solve: restarts > 0 needs refine > 0 (the sweeps of every replica)")
        if refine < 0:
            raise ValueError("solve: refine must be >= 0")
        if exchanges < 0:
            raise ValueError("solve: exchanges must be >= 0")
        if exchanges > 0 and refine == 0:
            raise ValueError("solve: exchanges > 0 needs refine > 0 (the sweeps between the exchanges)")
        K = self.K
        scenes, S, seed, limits = self._prepare("solve", scenes, num_scenes, seed, constraints, (
            (constraints is not None and refine == 0,
             "solve: constraints need refine > 0 (the decode ignores them; the search applies them)"),
            (starts == "replicas" and K < 2,
             f"solve: starts='replicas' needs samples >= 2 (got {K}: one replica is starts='best')"),
            (starts == "replicas" and restarts < K,  # so restarts > 0: refine > 0
             f"solve: starts='replicas' needs restarts={restarts} >= samples={K} (one replica of the search per "
             f"decoded replica)")))
        with torch.cuda.device(self.device):
            env = self._scene_env(scenes, S, seed)
            r = self._decode(env, S, seed, max_steps, trace)
            start_J = None
            if refine > 0 and starts == "replicas":
                allowed, capacity, fixed_ids = limits or (None, None, None)
                given = env.assigned_target_ids().to(torch.int32).view(S, K, self.N)  # scene-major already: no gather
                given, fixed = _with_fixed(given, fixed_ids, None, env.device)
                start_J = torch.empty(S, restarts, dtype=torch.float64, device=env.device)
                found = env.search_assignments_multistart(
                    None, allowed, fixed, capacity, restarts=restarts, seed=seed & (2 ** 64 - 1), stride=K, rows=S,
                    max_exchanges=exchanges, max_sweeps=refine, J_all=start_J, starts=given.contiguous())
            elif refine > 0:
                found = self._search(env, r.assignment, S, refine, exchanges, restarts, seed, limits)
            if refine > 0:
                r = replace(r, assignment=found[0], J=found[1], covered=found[2], decoded_J=r.J, refine_stats=found[3],
                            start_J=start_J)
            return self._lns(env, r, S, seed, lns_rounds, lns_free, lns_mode, limits)

    @torch.no_grad()
    def baseline(self, scenes=None, num_scenes=None, seed=None, max_sweeps=32, exchanges=0, constraints=None,
                 restarts=0, lns_rounds=0, lns_free=12, lns_mode="targets"):
        """The non-learned yardstick for the same objective: the scenes solve() would run (scene for
        scene under the same `seed`), no policy launch, the best-response local search started from
        the empty assignment (a greedy constructor plus local search). Returns an Allocation whose
        decode-only fields (best_replica, steps, replica_J) are zeros. exchanges = X > 0: the search
        with at most X pairwise exchanges (uavhip_search_assignments), refine_stats [S, 6].
        constraints = Constraints(...): uavhip_search_assignments_constrained from the assignment that
        holds the committed UAVs' fixed ids and nothing else, refine_stats [S, 8].
        restarts = R > 0: uavhip_search_multistart with R replicas -- replica 0 the search this call would
        run without it, the others from random full assignments drawn with Philox key `seed` -- and the
        best J per scene, refine_stats [S, 10]. restarts = 0 launches nothing new and changes no result.
        lns_rounds = L > 0: then L rounds of the large-neighbourhood search from that result, as solve's;
        lns_J_before is the J going in. lns_rounds = 0 launches nothing more and changes nothing."""
        exchanges, restarts, lns_rounds, lns_free = int(exchanges), int(restarts), int(lns_rounds), int(lns_free)
        _check_lns("baseline", lns_rounds, lns_free, lns_mode)
        if exchanges < 0:
            raise ValueError("baseline: exchanges must be >= 0")
        if not 0 <= restarts <= _lib.MULTISTART_MAX_R:
            raise ValueError(f"baseline: restarts must be in [0, {_lib.MULTISTART_MAX_R}]")
        scenes, S, seed, limits = self._prepare("baseline", scenes, num_scenes, seed, constraints)
        with torch.cuda.device(self.device):
            env = self._scene_env(scenes, S, seed)
            found = self._search(env, None, S, max_sweeps, exchanges, restarts, seed, limits)
            return self._lns(env, self._undecoded(env, S, *found), S, seed, lns_rounds, lns_free, lns_mode, limits)

    @torch.no_grad()
    def optimum(self, scenes=None, num_scenes=None, seed=None, constraints=None, max_workspace_bytes=1 << 30):
        """The best allocation there is: the scenes solve() / baseline() would run (scene for scene
        under the same `seed`), no policy launch, the maximum of J over every allocation by a subset DP
        over the UAVs (uavhip_solve_exact; N <= 16, 3^N steps a target). Returns an Allocation whose
        decode-only fields are zeros, as baseline's; refine_stats is [S, 2]: invalid ids, fixed conflicts.
        constraints = Constraints(...): the maximum over the allocations baseline(constraints=) may end
        on -- committed UAVs where they are, allowed pairs only, capacities kept."""
        scenes, S, seed, limits = self._prepare("optimum", scenes, num_scenes, seed, constraints, ((
            self.N > _lib.EXACT_MAX_N,
            f"optimum: N={self.N} > {_lib.EXACT_MAX_N} (the subset DP takes 3^N steps a target)"),))
        allowed, capacity, fixed_ids = limits or (None, None, None)
        with torch.cuda.device(self.device):
            env = self._scene_env(scenes, S, seed)
            start, fixed = _with_fixed(None, fixed_ids, (S, self.N), env.device)
            found = env.exact_assignments(start, allowed, fixed, capacity, stride=self.K, rows=S,
                                          max_workspace_bytes=max_workspace_bytes)
            return self._undecoded(env, S, *found)


def main(argv=None):
    import argparse
    import json
    import time

    from .checkpoint import load_checkpoint
    from .policy import TransformerActorCritic
    ap = argparse.ArgumentParser(description="Decode allocations for on-device scenes with a trained policy")
    ap.add_argument("--checkpoint", required=True, help="a torch.save(policy.state_dict()) file (main_train.py:211)")
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--uavs", type=int, default=default_cfg.NUM_UAVS)
    ap.add_argument("--targets", type=int, default=default_cfg.NUM_TARGETS)
    ap.add_argument("--refine", type=int, default=0, metavar="SWEEPS",
                    help="polish each allocation by at most SWEEPS sweeps of the best-response local search on J")
    ap.add_argument("--exchanges", type=int, default=0, metavar="X",
                    help="with --refine: at most X pairwise exchanges between the sweeps (uavhip_search_assignments); "
                         "with --baseline: also the baseline with exchanges, beside the plain one")
    ap.add_argument("--baseline", action="store_true",
                    help="also run the non-learned baseline (the local search from the empty assignment) on the "
                         "same scenes and report the share of scenes where the policy's J is larger")
    ap.add_argument("--optimum", action="store_true",
                    help="also the optimum of J on the same scenes (a subset DP over the UAVs, --uavs <= 16) and every "
                         "mean J's share of it; implies --baseline")
    ap.add_argument("--restarts", type=int, default=0, metavar="R",
                    help="also the baseline as the best of R restarts of the exchange search (uavhip_search_multistart; "
                         "--exchanges' cap, or 32 when that is 0): mean_J_multistart; implies --baseline")
    ap.add_argument("--starts", choices=("best", "replicas"), default="best",
                    help="replicas (needs --restarts R >= --samples K >= 2): also the search started from all K decoded "
                         "replicas of each scene plus R - K random starts (uavhip_search_multistart_from; --refine's and "
                         "--exchanges' caps, 32 where they are 0): mean_J_policy_starts, policy_start_wins, "
                         "policy_starts_beat_random")
    ap.add_argument("--lns", type=int, default=0, metavar="ROUNDS",
                    help="also the baseline (--exchanges' cap, or 32 when that is 0) followed by ROUNDS rounds of the "
                         "large-neighbourhood search (uavhip_solve_exact_free on --lns-free UAVs a round): mean_J_lns, "
                         "lns_improved; implies --baseline")
    ap.add_argument("--lns-free", type=int, default=12, metavar="K", help="the UAVs freed per round of --lns, 1..16")
    ap.add_argument("--lns-mode", choices=("random", "targets"), default="targets",
                    help="how a round of --lns chooses them: by random keys, or the idle UAVs and the crews of random targets")
    a = ap.parse_args(argv)
    if a.lns < 0:
        ap.error("--lns must be >= 0")
    if not 1 <= a.lns_free <= _lib.EXACT_FREE_MAX:
        ap.error(f"--lns-free must be in [1, {_lib.EXACT_FREE_MAX}]")
    if a.exchanges < 0:
        ap.error("--exchanges must be >= 0")
    if not 0 <= a.restarts <= _lib.MULTISTART_MAX_R:
        ap.error(f"--restarts must be in [0, {_lib.MULTISTART_MAX_R}]")
    if a.starts == "replicas" and not 2 <= a.samples <= a.restarts:
        ap.error("--starts replicas needs --restarts R >= --samples K >= 2")
    if a.optimum and a.uavs > _lib.EXACT_MAX_N:
        ap.error(f"--optimum needs --uavs <= {_lib.EXACT_MAX_N} (the subset DP takes 3^N steps a target)")
    if not torch.cuda.is_available():
        raise RuntimeError("uavhip.solve decodes on the GPU (HIP) only")
    dev = torch.device("cuda:0")
    policy = TransformerActorCritic().to(dev)
    load_checkpoint(policy, a.checkpoint)
    solver = AllocationSolver(policy, a.uavs, a.targets, samples=a.samples)
    on = dict(num_scenes=a.scenes, seed=a.seed)
    ex = a.exchanges if a.refine > 0 else 0  # without --refine, --exchanges is the baseline's alone
    solver.solve(**on, refine=a.refine, exchanges=ex)  # warm-up: allocation, weight pack
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = solver.solve(**on, refine=a.refine, exchanges=ex)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    r = r.cpu()
    out = {"scenes": a.scenes, "samples": a.samples, "N": a.uavs, "M": a.targets, "seed": a.seed,
           "mean_J": float(r.J.mean()), "best_J": float(r.J.max()),
           "mean_covered": float(r.covered.double().mean()), "mean_steps": float(r.steps.double().mean()),
           "unfinished": int((r.best_replica < 0).sum()), "scenes_per_s": a.scenes / dt}
    if a.refine > 0:
        out.update(mean_J_decoded=float(r.decoded_J.mean()), mean_J_refined=float(r.J.mean()))
        if a.exchanges > 0:
            out.update(mean_exchanges=float(r.refine_stats[:, 4].double().mean()))
    rivals = {}  # name -> Allocation: what --optimum reports as name_over_optimal and name_is_optimal, in this order
    if a.baseline or a.optimum or a.restarts > 0 or a.lns > 0:
        b = solver.baseline(**on).cpu()
        out.update(mean_J_baseline=float(b.J.mean()), policy_beats_baseline=float((r.J > b.J).double().mean()))
        if a.exchanges > 0:
            bx = rivals["baseline_exchange"] = solver.baseline(**on, exchanges=a.exchanges).cpu()
            out.update(mean_J_baseline_exchange=float(bx.J.mean()))
        if a.restarts > 0:
            bm = rivals["multistart"] = solver.baseline(**on, exchanges=a.exchanges or 32, restarts=a.restarts).cpu()
            out.update(mean_J_multistart=float(bm.J.mean()))
        if a.starts == "replicas":
            ps = rivals["policy_starts"] = solver.solve(**on, refine=a.refine or 32, exchanges=a.exchanges or 32,
                                                        restarts=a.restarts, starts="replicas").cpu()
            out.update(mean_J_policy_starts=float(ps.J.mean()),
                       policy_start_wins=float((ps.refine_stats[:, 8] < a.samples).double().mean()),
                       policy_starts_beat_random=float((ps.J > bm.J).double().mean()))
        if a.lns > 0:
            bl = rivals["lns"] = solver.baseline(**on, exchanges=a.exchanges or 32, lns_rounds=a.lns, lns_free=a.lns_free,
                                                 lns_mode=a.lns_mode).cpu()
            out.update(mean_J_lns=float(bl.J.mean()), lns_improved=float((bl.J > bl.lns_J_before).double().mean()))
    if a.optimum:
        o = solver.optimum(**on).cpu()
        best = float(o.J.mean())

        over = lambda J: float(J.mean()) / best  # noqa: E731
        reaches = lambda x: float((x.J >= o.J - RTOL * o.J.abs().clamp(min=1.0)).double().mean())  # noqa: E731
        out.update(mean_J_optimal=best, baseline_over_optimal=over(b.J))
        if a.refine > 0:
            out.update(decoded_over_optimal=over(r.decoded_J), refined_over_optimal=over(r.J))
        else:
            out.update(decoded_over_optimal=over(r.J))
        out.update(baseline_is_optimal=reaches(b))
        for name, x in rivals.items():
            out.update({f"{name}_over_optimal": over(x.J), f"{name}_is_optimal": reaches(x)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
