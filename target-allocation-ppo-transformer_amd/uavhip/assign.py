"""The allocators on J(X) of libuavhip.so (include/uavhip.h), which VecUAVEnv (vec_env.py) inherits from
AssignmentSolvers: select_best, the local searches, the exact solvers and the large-neighbourhood search. They
only read the env. Their argument handling is module-level, each check written once: the checks run on any
object with the attributes they read (E, N, M, device), before any device call."""
import torch

from . import _lib
from ._lib import LIB, check, check_out, out_buf, ptr, stream_handle


def _rows_args(fn, E, stride, rows, **non_negative):
    """The row arguments refine_assignments and search_assignments (`fn`) share: row s on the scene
    of env s * stride, `rows` of them (None: every stride-th of the E envs), and the caps, each
    >= 0. -> the number of rows."""
    if stride < 1:
        raise ValueError(f"{fn}: stride={stride} must be >= 1")
    S = (E - 1) // stride + 1 if rows is None else int(rows)
    if S < 1 or (S - 1) * stride >= E:
        raise ValueError(f"{fn}: rows={S} at stride={stride} do not fit E={E}")
    for name, cap in non_negative.items():
        if cap < 0:
            raise ValueError(f"{fn}: {name}={cap} must be >= 0")
    return S


def _rows_bufs(S, N, n_stats, dev, assignment, out, J, covered, stats):
    """Their buffers: the given `assignment` checked, the four outputs given or allocated."""
    check_out(assignment, "assignment", torch.int32, (S, N), dev)
    return (out_buf(out, "out", torch.int32, (S, N), dev), out_buf(J, "J", torch.float64, (S,), dev),
            out_buf(covered, "covered", torch.int32, (S,), dev), out_buf(stats, "stats", torch.int32, (S, n_stats), dev))


def _check_limits(env, S, allowed, fixed, capacity):
    """The three constraint arrays, indexed by row; None passes."""
    check_out(allowed, "allowed", torch.uint8, (S, env.N, env.M), env.device)
    check_out(fixed, "fixed", torch.uint8, (S, env.N), env.device)
    check_out(capacity, "capacity", torch.int32, (S, env.M), env.device)


def _check_free(fn, name, K, why=""):
    """The free UAVs of a subset DP, argument `name`."""
    if not 1 <= K <= _lib.EXACT_FREE_MAX:
        raise ValueError(f"{fn}: {name}={K} must be in [1, {_lib.EXACT_FREE_MAX}]{why}")


def _check_bits(fn, name, value, bits):
    """A Philox key (seed, 64 bits) or counter word (round, 32 bits)."""
    if not 0 <= value < 2 ** bits:
        raise ValueError(f"{fn}: {name}={value} must be in [0, 2^{bits})")


def _check_mode(fn, mode, name="mode"):
    if mode not in _lib.NBH:
        raise ValueError(f"{fn}: {name} must be one of {sorted(_lib.NBH)} (got {mode!r})")


def _chunk_bytes(fn, S, row, max_bytes, what):
    """The workspace of a solver that runs S rows in chunks: `row` bytes a row (of `what`) and the cap
    (None: all rows at once) -> the bytes to allocate, for min(S, the rows that fit) rows."""
    fit = S if max_bytes is None else int(max_bytes) // row
    if fit < 1:
        raise ValueError(f"{fn}: max_workspace_bytes={max_bytes} holds no row (one row of {what} needs {row} bytes)")
    return row * min(S, fit)


def _kept_workspace(env, name, nbytes):
    """The env's own workspace tensor `name`, kept and reused while it is large enough."""
    ws = env.__dict__.get(name)  # not getattr: VecUAVEnv.__getattr__ is the scene arrays'
    if ws is None or ws.numel() < nbytes:
        ws = env.__dict__[name] = torch.empty(nbytes, dtype=torch.uint8, device=env.device)
    return ws


class AssignmentSolvers:
    def select_best(self, K, best=None, J=None, covered=None, assignment=None):
        """uavhip_select_best: the envs as K replicas of E / K scenes, scene-major (e = s * K + k).
        Per scene the finished replica with the largest J (lowest k on a tie): (best [S] int32, -1
        when none finished; J [S] f64; covered [S] int32; assignment [S, N] int32 target ids)."""
        K = int(K)
        if K <= 0 or self.E % K:
            raise ValueError(f"select_best: K={K} must be > 0 and divide E={self.E}")
        S, dev = self.E // K, self.device
        best = out_buf(best, "best", torch.int32, (S,), dev)
        J = out_buf(J, "J", torch.float64, (S,), dev)
        covered = out_buf(covered, "covered", torch.int32, (S,), dev)
        assignment = out_buf(assignment, "assignment", torch.int32, (S, self.N), dev)
        check(LIB.uavhip_select_best(self.desc, K, ptr(best), ptr(J), ptr(covered), ptr(assignment), stream_handle()),
              "uavhip_select_best")
        return best, J, covered, assignment

    def refine_assignments(self, assignment=None, stride=1, rows=None, max_sweeps=32, out=None, J=None, covered=None,
                           stats=None):
        """uavhip_refine_assignments: best-response local search on J(X) for `rows` scenes, row s on
        the scene of env s * stride (rows defaults to every stride-th env; stride = K after
        select_best(K)). assignment [rows, N] int32 target ids or -1 (None: start from the empty
        assignment -- a greedy constructor plus local search); max_sweeps = 0 only scores it.
        Returns (assignment [rows, N] int32 target ids, J [rows] f64, covered [rows] int32,
        stats [rows, 4] int32: sweeps, moves, converged, invalid input ids). out may be `assignment`
        itself (in place). The env is only read."""
        stride, max_sweeps = int(stride), int(max_sweeps)
        S = _rows_args("refine_assignments", self.E, stride, rows, max_sweeps=max_sweeps)
        out, J, covered, stats = _rows_bufs(S, self.N, 4, self.device, assignment, out, J, covered, stats)
        check(LIB.uavhip_refine_assignments(self.desc, stride, S, max_sweeps, ptr(assignment), ptr(out), ptr(J),
                                            ptr(covered), ptr(stats), stream_handle()), "uavhip_refine_assignments")
        return out, J, covered, stats

    def search_assignments(self, assignment=None, stride=1, rows=None, max_exchanges=32, max_sweeps=32, out=None,
                           J=None, covered=None, stats=None):
        """uavhip_search_assignments: refine_assignments' best-response search plus the pairwise
        exchange -- where no single move improves J, the best swap of two UAVs' targets (one may be
        "none") is made and the sweeps run again, at most max_exchanges times, max_sweeps sweeps per
        phase. Arguments as refine_assignments. Returns (assignment [rows, N] int32 target ids,
        J [rows] f64, covered [rows] int32, stats [rows, 6] int32: sweeps, moves, the last phase
        converged, invalid input ids, exchanges made, 1 if the last scan found no improving pair).
        max_exchanges = 0 is refine_assignments, bitwise. The env is only read."""
        stride, max_exchanges, max_sweeps = int(stride), int(max_exchanges), int(max_sweeps)
        S = _rows_args("search_assignments", self.E, stride, rows, max_exchanges=max_exchanges, max_sweeps=max_sweeps)
        out, J, covered, stats = _rows_bufs(S, self.N, 6, self.device, assignment, out, J, covered, stats)
        check(LIB.uavhip_search_assignments(self.desc, stride, S, max_exchanges, max_sweeps, ptr(assignment), ptr(out),
                                            ptr(J), ptr(covered), ptr(stats), stream_handle()),
              "uavhip_search_assignments")
        return out, J, covered, stats

    def search_assignments_constrained(self, assignment=None, allowed=None, fixed=None, capacity=None, stride=1,
                                       rows=None, max_exchanges=32, max_sweeps=32, out=None, J=None, covered=None,
                                       stats=None):
        """uavhip_search_assignments_constrained: search_assignments under three constraints, each
        indexed by ROW with its columns in list order (as p_dmg's), None for "no such constraint":
        allowed [rows, N, M] uint8 (nonzero: the UAV may take the target), fixed [rows, N] uint8
        (nonzero: the UAV keeps the target `assignment` gives it, or none) and capacity [rows, M]
        int32 (the most UAVs on the target; < 0 counts as 0). A free UAV's input pair that is not
        allowed, or whose target is full, is dropped before the search. Other arguments as
        search_assignments. Returns (assignment [rows, N] int32 target ids, J [rows] f64, covered
        [rows] int32, stats [rows, 8] int32: search_assignments' six, pairs dropped at the start,
        conflicts of the fixed UAVs with allowed / capacity). Without constraints, or with neutral
        ones, it is search_assignments, bitwise. The env is only read."""
        stride, max_exchanges, max_sweeps = int(stride), int(max_exchanges), int(max_sweeps)
        S = _rows_args("search_assignments_constrained", self.E, stride, rows, max_exchanges=max_exchanges, max_sweeps=max_sweeps)
        _check_limits(self, S, allowed, fixed, capacity)
        out, J, covered, stats = _rows_bufs(S, self.N, 8, self.device, assignment, out, J, covered, stats)
        check(LIB.uavhip_search_assignments_constrained(self.desc, stride, S, max_exchanges, max_sweeps, ptr(allowed),
                                                        ptr(fixed), ptr(capacity), ptr(assignment), ptr(out), ptr(J),
                                                        ptr(covered), ptr(stats), stream_handle()),
              "uavhip_search_assignments_constrained")
        return out, J, covered, stats

    def exact_assignments(self, assignment=None, allowed=None, fixed=None, capacity=None, stride=1, rows=None, out=None,
                          J=None, covered=None, stats=None, max_workspace_bytes=1 << 30):
        """uavhip_solve_exact: the optimum of J(X) by a subset DP over the UAVs, N <= 16 (3^N steps a
        target; include/uavhip.h has the rule and the tie-break). Rows, stride and the three constraint
        arrays are search_assignments_constrained's, and the feasible set is its guarantee: a fixed UAV
        stays where `assignment` puts it (it is read for nothing else, and required with `fixed`), a
        free UAV takes allowed pairs only, no target holds more than max(capacity, its fixed UAVs).
        The workspace (5 MiB a row at 16 x 32) is allocated for min(rows, what fits in
        max_workspace_bytes) rows; more rows run in chunks, one after the other.
        Returns (assignment [rows, N] int32 target ids, J [rows] f64, covered [rows] int32, stats
        [rows, 2] int32: invalid input ids, conflicts of the fixed UAVs with allowed / capacity). J is
        refine_assignments(assignment, max_sweeps=0)'s, bitwise. The env is only read."""
        fn = "exact_assignments"
        stride = int(stride)
        S = _rows_args(fn, self.E, stride, rows)
        if self.N > _lib.EXACT_MAX_N:
            raise ValueError(f"{fn}: N={self.N} > {_lib.EXACT_MAX_N} (the subset DP takes 3^N steps a target)")
        if fixed is not None and assignment is None:
            raise ValueError(f"{fn}: fixed needs assignment (a fixed UAV keeps the target it gives)")
        _check_limits(self, S, allowed, fixed, capacity)
        out, J, covered, stats = _rows_bufs(S, self.N, 2, self.device, assignment, out, J, covered, stats)
        nbytes = _chunk_bytes(fn, S, int(LIB.uavhip_exact_workspace_bytes(self.N, self.M, 1)), max_workspace_bytes,
                              f"{self.N} x {self.M}")
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)  # a fresh one per call
        check(LIB.uavhip_solve_exact(self.desc, stride, S, ptr(allowed), ptr(fixed), ptr(capacity), ptr(assignment),
                                     ptr(out), ptr(J), ptr(covered), ptr(stats), ptr(workspace), nbytes,
                                     stream_handle()), "uavhip_solve_exact")
        return out, J, covered, stats

    def exact_free_assignments(self, assignment=None, *, max_free, allowed=None, fixed=None, capacity=None, stride=1,
                               rows=None, out=None, J=None, covered=None, stats=None, max_workspace_bytes=None):
        """uavhip_solve_exact_free: exact_assignments' subset DP over a row's FREE UAVs only -- those with
        fixed == 0, the first max_free (1..16) of them in ascending order; any further free UAV is held
        like a fixed one -- for every N <= 64, M <= 128. A held UAV stays where `assignment` puts it (None:
        on none) and only scales its target's value, so the row's result is the best of the (M + 1)^K
        assignments of its K free UAVs: never below `assignment`'s J when that is feasible. Rows, stride
        and the three constraint arrays are exact_assignments'; include/uavhip.h has the rule.
        The workspace is the env's own tensor, kept and reused while it is large enough (so the call can
        be captured in a graph after one eager call); max_workspace_bytes (None: all rows at once) caps it,
        and more rows than fit run in chunks.
        Returns (assignment [rows, N] int32 target ids, J [rows] f64, covered [rows] int32, stats
        [rows, 4] int32: invalid input ids, conflicts of the held UAVs with allowed / capacity, free UAVs
        in the DP, free UAVs held by overflow). out may be `assignment` itself. The env is only read."""
        fn = "exact_free_assignments"
        stride, K = int(stride), int(max_free)
        S = _rows_args(fn, self.E, stride, rows)
        _check_free(fn, "max_free", K, " (the subset DP takes 3^max_free steps a target)")
        if fixed is not None and assignment is None:
            raise ValueError(f"{fn}: fixed needs assignment (a held UAV keeps the target it gives)")
        _check_limits(self, S, allowed, fixed, capacity)
        out, J, covered, stats = _rows_bufs(S, self.N, 4, self.device, assignment, out, J, covered, stats)
        nbytes = _chunk_bytes(fn, S, int(LIB.uavhip_exact_free_workspace_bytes(min(K, self.N), self.M, 1)),
                              max_workspace_bytes, f"{min(K, self.N)} free UAVs x {self.M} targets")
        ws = _kept_workspace(self, "_exact_free_ws", nbytes)
        check(LIB.uavhip_solve_exact_free(self.desc, stride, S, K, ptr(allowed), ptr(fixed), ptr(capacity),
                                          ptr(assignment), ptr(out), ptr(J), ptr(covered), ptr(stats), ptr(ws), nbytes,
                                          stream_handle()), "uavhip_solve_exact_free")
        return out, J, covered, stats

    def pick_neighbourhood(self, assignment, K, mode, round, seed, fixed=None, stride=1, rows=None, out=None):
        """uavhip_neighbourhood_pick: the free set of one round of a large-neighbourhood search, chosen
        on device. -> fixed_out [rows, N] uint8, 1 = held: the UAVs with `fixed` != 0 always, and of the
        others all but the first K (1..16) by the mode's Philox key under (`seed`, `round`): mode
        "random" sorts the UAVs by their own keys; "targets" frees the idle UAVs first, then the whole
        crews of targets in a random order (`assignment` [rows, N] int32 target ids or -1; None: all
        idle). include/uavhip.h has the rule. The result is exact_free_assignments' `fixed`. The env is
        only read."""
        fn = "pick_neighbourhood"
        stride, K, round, seed = int(stride), int(K), int(round), int(seed)
        S = _rows_args(fn, self.E, stride, rows)
        _check_free(fn, "K", K)
        _check_mode(fn, mode)
        _check_bits(fn, "round", round, 32)
        _check_bits(fn, "seed", seed, 64)
        check_out(assignment, "assignment", torch.int32, (S, self.N), self.device)
        check_out(fixed, "fixed", torch.uint8, (S, self.N), self.device)
        out = out_buf(out, "out", torch.uint8, (S, self.N), self.device)
        check(LIB.uavhip_neighbourhood_pick(self.desc, stride, S, K, _lib.NBH[mode], round, seed, ptr(assignment),
                                            ptr(fixed), ptr(out), stream_handle()), "uavhip_neighbourhood_pick")
        return out

    def lns_assignments(self, assignment, *, rounds, free, mode="targets", seed=0, allowed=None, fixed=None,
                        capacity=None, stride=1, rows=None):
        """Large-neighbourhood search on J: `rounds` times, pick_neighbourhood(K = free, mode, round r,
        seed) chooses the row's free UAVs, exact_free_assignments solves that neighbourhood to optimality,
        and the row keeps the new result only where its J is strictly greater than the one it holds --
        compared on the doubles themselves, so J never decreases and is never below the start's.
        `assignment` [rows, N] int32 target ids or -1 is the start (not written); the UAVs with `fixed`
        != 0 never move, `allowed` / `capacity` bind the free UAVs of every round (a start that breaks
        them is kept where held: start from a search under the same constraints). Everything is ordered
        on the current stream with no host synchronisation; after one eager call (which sizes the env's
        workspace) the call can be captured in a graph.
        Returns (assignment [rows, N] int32 target ids, J [rows] f64, covered [rows] int32, improved
        [rows] int32: the rounds that raised the row's J). The env is only read."""
        fn = "lns_assignments"
        rounds, K, seed, stride = int(rounds), int(free), int(seed), int(stride)
        S = _rows_args(fn, self.E, stride, rows, rounds=rounds)
        _check_free(fn, "free", K)
        _check_mode(fn, mode)
        _check_bits(fn, "seed", seed, 64)
        if assignment is None:
            raise ValueError(f"{fn}: assignment is required ([rows, N] int32 target ids or -1: the start)")
        check_out(assignment, "assignment", torch.int32, (S, self.N), self.device)
        _check_limits(self, S, allowed, fixed, capacity)
        # the start scored and written as the library writes ids (an id of no target becomes -1)
        best, bJ, bcov, _ = self.refine_assignments(assignment, stride=stride, rows=S, max_sweeps=0)
        improved = torch.zeros(S, dtype=torch.int32, device=self.device)
        held = torch.empty(S, self.N, dtype=torch.uint8, device=self.device)
        new = tuple(torch.empty_like(t) for t in (best, bJ, bcov))
        for r in range(rounds):
            self.pick_neighbourhood(best, K, mode, r, seed, fixed=fixed, stride=stride, rows=S, out=held)
            self.exact_free_assignments(best, max_free=K, allowed=allowed, fixed=held, capacity=capacity,
                                        stride=stride, rows=S, out=new[0], J=new[1], covered=new[2])
            up = new[1] > bJ
            best = torch.where(up[:, None], new[0], best)
            bJ = torch.where(up, new[1], bJ)
            bcov = torch.where(up, new[2], bcov)
            improved = improved + up.to(torch.int32)
        return best, bJ, bcov, improved

    def search_assignments_multistart(self, assignment=None, allowed=None, fixed=None, capacity=None, restarts=16,
                                      seed=0, stride=1, rows=None, max_exchanges=32, max_sweeps=32, out=None, J=None,
                                      covered=None, stats=None, J_all=None, starts=None):
        """uavhip_search_multistart: per row the best of `restarts` = R independent runs (replicas) of
        search_assignments_constrained -- replica 0 from `assignment` (its result bit for bit), the
        others from uniform random full assignments drawn with Philox key `seed` (a fixed UAV keeps
        the target `assignment` gives it in every replica); the caps hold per replica and the replica
        with the largest J wins, the lowest index among equal J (include/uavhip.h has the rule). Rows,
        stride and the three constraint arrays are search_assignments_constrained's, None included.
        starts [rows, R0, N] int32 target ids or -1, instead of `assignment` (uavhip_search_multistart_from):
        replicas 0 .. R0 - 1 run from the row's R0 given starts, each the constrained search from its
        own start, and replicas R0 .. R - 1 are the random ones, replica r what it is without `starts`;
        a fixed UAV keeps the target starts[:, 0] gives it in every replica. Needs restarts >= R0.
        Without `starts` the call is what it was, launch for launch.
        Returns (assignment [rows, N] int32 target ids, J [rows] f64, covered [rows] int32, stats
        [rows, 10] int32: the chosen replica's eight counters of the constrained search, its index,
        the number of replicas strictly above replica 0's J). J_all [rows, R] f64, when given, receives
        every replica's J. 1 <= R <= 1024. The workspace (44 + 4 N bytes a replica) is the env's own
        tensor, kept and reused while it is large enough. out may be `assignment` itself. The env is
        only read."""
        stride, max_exchanges, max_sweeps, R = int(stride), int(max_exchanges), int(max_sweeps), int(restarts)
        fn = "search_assignments_multistart"
        S = _rows_args(fn, self.E, stride, rows, max_exchanges=max_exchanges, max_sweeps=max_sweeps)
        if not 1 <= R <= _lib.MULTISTART_MAX_R:
            raise ValueError(f"{fn}: restarts={R} must be in [1, {_lib.MULTISTART_MAX_R}]")
        seed = int(seed)
        _check_bits(fn, "seed", seed, 64)
        R0 = 0
        if starts is not None:
            if assignment is not None:
                raise ValueError(f"{fn}: pass assignment or starts, not both")
            ok = isinstance(starts, torch.Tensor) and starts.dim() == 3 and starts.shape[1] >= 1 and \
                tuple(starts.shape[::2]) == (S, self.N)
            if ok:
                check_out(starts, "starts", torch.int32, starts.shape, self.device)
            else:
                got = f"{starts.dtype} {tuple(starts.shape)}" if isinstance(starts, torch.Tensor) else type(starts).__name__
                raise ValueError(f"starts: need a contiguous torch.int32 tensor [{S}, R0 >= 1, {self.N}] on {self.device} "
                                 f"(got {got})")
            R0 = int(starts.shape[1])
            if R < R0:
                raise ValueError(f"{fn}: restarts={R} must be >= the {R0} given starts")
        _check_limits(self, S, allowed, fixed, capacity)
        check_out(J_all, "J_all", torch.float64, (S, R), self.device)
        nbytes = int(LIB.uavhip_multistart_workspace_bytes(S, R, self.N))
        if nbytes < 0:
            raise ValueError(f"{fn}: rows={S} x restarts={R} is more than 2^30 replicas")
        out, J, covered, stats = _rows_bufs(S, self.N, 10, self.device, assignment, out, J, covered, stats)
        ws = _kept_workspace(self, "_multistart_ws", nbytes)
        if starts is not None:
            check(LIB.uavhip_search_multistart_from(self.desc, stride, S, R, R0, seed, max_exchanges, max_sweeps,
                                                    ptr(allowed), ptr(fixed), ptr(capacity), ptr(starts), ptr(out),
                                                    ptr(J), ptr(covered), ptr(stats), ptr(J_all), ptr(ws), ws.numel(),
                                                    stream_handle()), "uavhip_search_multistart_from")
        else:
            check(LIB.uavhip_search_multistart(self.desc, stride, S, R, seed, max_exchanges, max_sweeps, ptr(allowed),
                                               ptr(fixed), ptr(capacity), ptr(assignment), ptr(out), ptr(J), ptr(covered),
                                               ptr(stats), ptr(J_all), ptr(ws), ws.numel(), stream_handle()),
                  "uavhip_search_multistart")
        return out, J, covered, stats
