"""Host-side checks of uavhip_solve_exact (no GPU): exact_np, the subset DP of include/uavhip.h in
numpy with the three constraints, which tests/test_gpu_exact.py compares the kernel's J against;
brute_np, the plain enumeration of every feasible assignment, which exact_np is checked against
where (M + 1)^N can be enumerated; exact_np never below the exchange search; and the argument
checks of the entry point, of the Python layers above it and of the command line."""
import ctypes
import functools
import json

import numpy as np
import pytest

import capi_host
from test_constrained_search_host import check_guarantees, constrained_search_np, random_constraints, with_fixed
from test_refine_host import OMEGAS, RTOL_J, J_of, _env_desc, host_scenes
from test_search_host import _HostEnv, oracle_tables, search_np

_entry_point = capi_host._entry_point("uavhip_solve_exact")


def _P(p_dmg, p_pen):
    return np.asarray(p_dmg, np.float64) * np.asarray(p_pen, np.float64)[:, None]


def convert_ids(tgt_id, start, N):
    """ids -> list indices as the kernels convert them: the lowest list index of an id, -1 for -1 and
    for an id of no target."""
    ids = [int(x) for x in tgt_id]
    a = [-1] * N
    if start is not None:
        a = [ids.index(int(w)) if int(w) in ids else -1 for w in start]
    return ids, a


def target_masks(N, M, a, allowed, fixed, capacity):
    """Per target t: (may, must, cap) -- the UAVs that may be on it (free and allowed, or fixed to it),
    the UAVs fixed to it, max(capacity, the fixed UAVs on it). The feasible T: must <= T <= may, |T| <= cap."""
    fx = [False] * N if fixed is None else [bool(x) for x in fixed]
    out = []
    for t in range(M):
        must = sum(1 << u for u in range(N) if fx[u] and a[u] == t)
        may = must | sum(1 << u for u in range(N) if not fx[u] and (allowed is None or allowed[u][t]))
        cap = N if capacity is None else max(0, int(capacity[t]))
        out.append((may, must, max(cap, bin(must).count("1"))))
    return out


@functools.lru_cache(maxsize=None)
def _ternary(N):
    """Every pair T <= S of N-bit sets, grouped by S ascending: (S \\ T [3^N], T [3^N], the start of each
    S's group [2^N], popcount of every set [2^N])."""
    code = np.arange(3 ** N, dtype=np.int64)
    S = np.zeros_like(code)
    T = np.zeros_like(code)
    for b in range(N):
        d = code % 3
        code //= 3
        S |= (d > 0).astype(np.int64) << b
        T |= (d == 2).astype(np.int64) << b
    order = np.argsort(S, kind="stable")
    S, T = S[order], T[order]
    sets = np.arange(1 << N)
    pop = sum((sets >> b) & 1 for b in range(N))
    return S ^ T, T, np.searchsorted(S, sets), pop


def exact_np(p_dmg, p_pen, value, cost, tgt_id, omega, start=None, allowed=None, fixed=None, capacity=None):
    """The optimum of J over the feasible assignments of one scene by the subset DP of the header
    (numpy doubles; the order of its additions is numpy's, not the kernel's). Scene arguments, start,
    allowed [N, M], fixed [N], capacity [M] as constrained_search_np.
    -> (assignment [N] int32 target ids, J of that assignment scored with J_of)."""
    N, M = np.shape(p_dmg)
    P, v, c, omega = _P(p_dmg, p_pen), np.asarray(value, np.float64), np.asarray(cost, np.float64), float(omega)
    ids, a = convert_ids(tgt_id, start, N)
    masks = target_masks(N, M, a, allowed, fixed, capacity)
    # the kernel's blocking, for memory's sake: LO low bits in one vector operation, the high bits looped
    LO = min(N, 10)
    nlo, nhi = 1 << LO, 1 << (N - LO)
    rest, sub, starts, _ = _ternary(LO)
    sets = np.arange(1 << N)
    pop = sum((sets >> b) & 1 for b in range(N))
    csum = np.zeros(1 << N)
    for u in range(N):
        csum += np.where(sets >> u & 1, omega * c[u], 0.0)
    D = [np.zeros(1 << N)]
    vals = []
    for t in range(M):
        q = np.ones(1 << N)
        for u in range(N):
            q *= np.where(sets >> u & 1, 1.0 - P[u][t], 1.0)
        may, must, cap = masks[t]
        val = v[t] * (1.0 - q) - csum
        val[((sets & ~may) != 0) | ((sets & must) != must) | (pop > cap)] = -np.inf
        vals.append(val)
        V, prev = val.reshape(nhi, nlo), D[-1].reshape(nhi, nlo)
        live = np.isfinite(V).any(1)
        new = np.full((nhi, nlo), -np.inf)
        for Sh in range(nhi):
            Ths = np.array([Th for Th in range(Sh + 1) if Th & ~Sh == 0 and live[Th]], np.int64)
            if len(Ths):
                new[Sh] = np.maximum.reduceat((prev[Sh ^ Ths][:, rest] + V[Ths][:, sub]).max(0), starts)
        D.append(new.reshape(-1))
    S, out = (1 << N) - 1, [-1] * N
    for t in range(M - 1, -1, -1):
        Ts = sets[(sets & ~S) == 0]
        cand = D[t][S ^ Ts] + vals[t][Ts]
        T = int(Ts[np.flatnonzero(cand == cand.max())[0]])  # the smallest T among the maxima
        for u in range(N):
            if T >> u & 1:
                out[u] = t
        S ^= T
    assert np.isfinite(D[M][-1])
    J = J_of(P, v, c, omega, out)
    assert abs(J - D[M][-1]) <= 1e-9 * max(1.0, abs(J)), (J, D[M][-1])
    return np.array([ids[t] if t >= 0 else -1 for t in out], np.int32), J


def brute_np(p_dmg, p_pen, value, cost, tgt_id, omega, start=None, allowed=None, fixed=None, capacity=None):
    """Plain enumeration: the largest J over every assignment in {-1, 0..M-1}^N that the header's three
    conditions admit. -> (assignment [N] int32 target ids, J scored with J_of, the number of feasible
    assignments)."""
    N, M = np.shape(p_dmg)
    P, v, c, omega = _P(p_dmg, p_pen), np.asarray(value, np.float64), np.asarray(cost, np.float64), float(omega)
    ids, a0 = convert_ids(tgt_id, start, N)
    A = np.stack([g.ravel() for g in np.indices((M + 1,) * N)], 1) - 1  # [(M + 1)^N, N]
    fx = np.zeros(N, bool) if fixed is None else np.asarray(fixed).astype(bool)
    ok = np.ones(len(A), bool)
    for u in range(N):
        if fx[u]:
            ok &= A[:, u] == a0[u]
        elif allowed is not None:
            ok &= (A[:, u] < 0) | np.asarray(allowed, bool)[u][np.maximum(A[:, u], 0)]
    J = -omega * ((A >= 0) * c[None, :]).sum(1)
    for t in range(M):
        on = A == t
        if capacity is not None:
            ok &= on.sum(1) <= max(max(0, int(capacity[t])), sum(1 for u in range(N) if fx[u] and a0[u] == t))
        J = J + v[t] * (1.0 - np.where(on, 1.0 - P[:, t][None, :], 1.0).prod(1))
    J[~ok] = -np.inf
    best = A[int(np.argmax(J))]
    return (np.array([ids[t] if t >= 0 else -1 for t in best], np.int32), J_of(P, v, c, omega, list(best)),
            int(ok.sum()))


def exact_rows(p_dmg, p_pen, value, cost, tgt_id, omega, starts=None, allowed=None, fixed=None, capacity=None):
    """exact_np over rows -> (assignment [S, N], J [S])."""
    pick = lambda x, s: None if x is None else x[s]  # noqa: E731
    rows = [exact_np(p_dmg[s], p_pen[s], value[s], cost[s], tgt_id[s], omega, pick(starts, s), pick(allowed, s),
                     pick(fixed, s), pick(capacity, s)) for s in range(len(p_dmg))]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def exact_stats(tgt_id, starts, allowed, fixed, capacity):
    """stats [S, 2] of uavhip_solve_exact restated: the invalid input ids and pass 1's fixed_conflicts,
    as constrained_search_np counts them (no sweep, no exchange)."""
    pick = lambda x, s: None if x is None else x[s]  # noqa: E731
    S, M = np.shape(tgt_id)
    N = np.shape(starts)[1] if starts is not None else 1
    out = np.zeros((S, 2), np.int32)
    for s in range(S):
        if starts is None:
            continue
        st = constrained_search_np(np.zeros((N, M)), np.ones(N), np.ones(M), np.ones(N), tgt_id[s], 0.0, starts[s],
                                   pick(allowed, s), pick(fixed, s), pick(capacity, s), 0, 0)[3]
        out[s] = (st[3], st[7])
    return out


def constraint_cases(N, M, E, seed=11):
    """The constraint sets of one shape: (label, start ids [E, N] or None, allowed, fixed, capacity)."""
    allowed, capacity, fixed_ids = random_constraints(N, M, E, seed)
    start, fixed = with_fixed(None, fixed_ids)
    odd = start.copy()
    odd_fixed = np.zeros_like(fixed)
    odd[:, 0], odd_fixed[:, 0] = -1, 1            # a UAV fixed to none
    if N > 1:
        odd[:, 1], odd_fixed[:, 1] = M + 3, 1     # and one fixed to an id of no target
    return [("unconstrained", None, None, None, None),
            ("all three", start, allowed, fixed, capacity),
            ("allowed alone", None, allowed, None, None),
            ("fixed alone", start, None, fixed, None),
            ("capacity alone", None, None, None, capacity),
            ("a negative and a zero capacity", None, None, None, np.where(capacity == 1, -1, capacity - 2).astype(np.int32)),
            ("fixed to none and to an invalid id", odd, allowed, odd_fixed, capacity)]


@pytest.mark.parametrize("N,M,E", [(4, 4, 6), (5, 7, 3)])
def test_exact_np_is_the_enumeration(N, M, E):
    """Every feasible assignment enumerated ((M + 1)^N: 625 and 32768): the DP's J is the enumeration's
    maximum to the reward bar, and the DP's assignment is feasible."""
    for omega in OMEGAS:
        tabs = oracle_tables(N, M, E, omega)
        for label, start, allowed, fixed, capacity in constraint_cases(N, M, E):
            pick = lambda x, s: None if x is None else x[s]  # noqa: E731
            n_feasible = 0
            for s in range(E):
                args = tuple(t[s] for t in tabs) + (omega, pick(start, s), pick(allowed, s), pick(fixed, s),
                                                    pick(capacity, s))
                asg, J = exact_np(*args)
                _, Jb, n = brute_np(*args)
                assert abs(J - Jb) <= RTOL_J * max(1.0, abs(Jb)), (label, omega, s, J, Jb)
                n_feasible += n
                check_guarantees((label, omega, s), asg[None], tabs[4][s][None], pick(start, s)[None] if start is not None
                                 else None, pick(allowed, s)[None] if allowed is not None else None,
                                 pick(fixed, s)[None] if fixed is not None else None,
                                 pick(capacity, s)[None] if capacity is not None else None)
            assert label != "unconstrained" or n_feasible == E * (M + 1) ** N
            assert label == "unconstrained" or n_feasible < E * (M + 1) ** N, label
            print(f"({N}, {M}) omega {omega} {label}: {n_feasible} feasible assignments over {E} scenes")


def test_exact_np_is_never_below_the_search():
    """N = 12, M = 24 (3^12 steps a target: the most the numpy DP is asked for): the optimum is never
    below the exchange search's J beyond rounding."""
    N, M, E = 12, 24, 4
    for omega in OMEGAS:
        tabs = oracle_tables(N, M, E, omega)
        _, J = exact_rows(*tabs, omega)
        Js = np.array([search_np(*(t[s] for t in tabs), omega)[1] for s in range(E)])
        print(f"omega {omega}: optimum {J}, search {Js}")
        assert bool((J >= Js - RTOL_J * np.maximum(1.0, np.abs(J))).all()), (omega, J, Js)


def test_exact_stats_restatement():
    N, M, E = 5, 7, 3
    tabs = oracle_tables(N, M, E, 0.0)
    _, start, allowed, fixed, capacity = constraint_cases(N, M, E)[6]
    st = exact_stats(tabs[4], start, allowed, fixed, capacity)
    assert bool((st[:, 0] == 1).all())  # the id M + 3
    assert not exact_stats(tabs[4], None, allowed, None, capacity).any()


def test_binding_signature():
    from uavhip import _lib
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    res, args = _lib._SIGS["uavhip_solve_exact"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), i32, i32] + [vp] * 9 + [i64, vp]
    assert _lib.LIB.uavhip_solve_exact.argtypes == args
    assert _lib._SIGS["uavhip_exact_workspace_bytes"] == (i64, [i32, i32, i32])
    assert _lib.LIB.uavhip_exact_workspace_bytes.restype is i64
    assert _lib.LIB.uavhip_abi_version() == 6 and _lib.EXACT_MAX_N == 16


def test_workspace_bytes():
    from uavhip import _lib
    need = _lib.LIB.uavhip_exact_workspace_bytes
    one = need(16, 32, 1)
    # two D tables of 2^16 doubles and the choice table [32][2^16] of uint16: 5 MiB, plus the targets' masks
    assert 5 << 20 <= one <= (5 << 20) + 4096 and one % 16 == 0
    assert need(16, 32, 7) == 7 * one and need(1, 1, 1) >= 2 * 2 * 8 + 2 * 2
    for bad in ((0, 4, 1), (17, 4, 1), (4, 0, 1), (4, 129, 1), (4, 4, 0), (-1, 4, 1), (4, 4, -3)):
        assert need(*bad) == -1, bad


def test_argument_checks_without_gpu():
    """Every documented misuse of uavhip_solve_exact returns UAVHIP_EINVAL with a message naming the
    function, before any HIP call (the placeholders would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_solve_exact, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_solve_exact"
    row = int(_lib.LIB.uavhip_exact_workspace_bytes(8, 4, 1))

    def call(env=None, stride=1, S=6, allowed=P, fixed=P, cap=P, ain=P, out=P, J=P, cov=P, stats=P, ws=P, nbytes=row):
        return fn(env or _env_desc(), stride, S, allowed, fixed, cap, ain, out, J, cov, stats, ws, nbytes, None)

    assert call(out=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(J=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(cov=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(stride=0) == -1 and name in err() and b"env_stride=0" in err()
    assert call(stride=-2) == -1 and name in err() and b"env_stride=-2" in err()
    assert call(S=0) == -1 and name in err() and b"S=0" in err()
    assert call(S=7) == -1 and name in err() and b"E=6" in err()              # rows past E
    assert call(stride=3, S=3) == -1 and name in err() and b"E=6" in err()    # (S - 1) * stride = 6 = E
    assert call(stride=1 << 30, S=1 << 30) == -1 and name in err()            # no 32-bit wrap of the product
    assert call(env=_env_desc(N=65)) == -1 and name in err() and b"bad env dims" in err()
    assert call(env=_env_desc(M=129)) == -1 and name in err() and b"bad env dims" in err()
    big = int(_lib.LIB.uavhip_exact_workspace_bytes(16, 4, 1))
    assert call(env=_env_desc(N=17), nbytes=1 << 40) == -1 and name in err() and b"N=17" in err()
    assert call(env=_env_desc(N=64), nbytes=1 << 40) == -1 and name in err() and b"N=64" in err()
    assert call(ain=None) == -1 and name in err() and b"fixed without assignment_in" in err()
    assert call(nbytes=row - 1) == -1 and name in err() and b"workspace" in err()   # one byte short of a row
    assert call(env=_env_desc(N=16), nbytes=big - 1) == -1 and name in err() and b"workspace" in err()
    assert call(nbytes=0) == -1 and name in err() and b"workspace" in err()
    assert call(nbytes=-5) == -1 and name in err() and b"workspace" in err()
    assert call(ws=None) == -1 and name in err() and b"workspace" in err()
    assert call(ws=ctypes.c_void_p(24)) == -1 and name in err() and b"aligned" in err()
    assert call(allowed=None, fixed=None, cap=None, ain=None, out=None) == -1 and name in err()
    assert fn(None, 1, 1, P, P, P, P, P, P, P, P, P, row, None) == -1 and name in err()


class _OnGpu:
    """Stands in for a device policy: only the device is looked at."""

    def parameters(self, recurse=True):
        import torch

        class P:
            device = torch.device("cuda", 0)
        return iter([P()])


def test_python_layers_refuse_before_any_device_call():
    import torch

    from uavhip import AllocationSolver, Constraints
    from uavhip.vec_env import VecUAVEnv
    E, N, M = 6, 4, 4
    call = lambda *a, **k: VecUAVEnv.exact_assignments(_HostEnv(E, N, M), *a, **k)  # noqa: E731
    with pytest.raises(ValueError, match="exact_assignments: stride=0"):
        call(stride=0)
    with pytest.raises(ValueError, match="exact_assignments: rows=7"):
        call(rows=7)
    with pytest.raises(ValueError, match="exact_assignments: rows=3 at stride=3"):
        call(stride=3, rows=3)
    with pytest.raises(ValueError, match="exact_assignments: N=17 > 16"):
        VecUAVEnv.exact_assignments(_HostEnv(E, 17, M))
    with pytest.raises(ValueError, match="exact_assignments: fixed needs assignment"):
        call(fixed=torch.zeros(E, N, dtype=torch.uint8))
    with pytest.raises(ValueError, match="assignment: need a contiguous torch.int32"):
        call(torch.zeros(E, N, dtype=torch.int64))
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8"):
        call(allowed=torch.ones(E, N, M, dtype=torch.bool))
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8 tensor of 48"):
        call(allowed=torch.ones(E, N, M, dtype=torch.uint8), stride=2)  # row-indexed: 3 rows at stride 2
    with pytest.raises(ValueError, match="fixed: need a contiguous torch.uint8"):
        call(torch.zeros(E, N, dtype=torch.int32), fixed=torch.zeros(E, N + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="capacity: need a contiguous torch.int32"):
        call(capacity=torch.zeros(E, M, dtype=torch.int64))
    with pytest.raises(ValueError, match="stats: need a contiguous torch.int32"):
        call(stats=torch.zeros(E, 8, dtype=torch.int32))  # the constrained search's shape
    with pytest.raises(ValueError, match="J: need a contiguous torch.float64"):
        call(J=torch.zeros(E, dtype=torch.float32))
    with pytest.raises(ValueError, match="max_workspace_bytes=100 holds no row"):
        call(max_workspace_bytes=100)

    S = 2
    s = AllocationSolver(_OnGpu(), N, M, samples=2)
    with pytest.raises(ValueError, match="optimum: pass scenes or num_scenes"):
        s.optimum()
    with pytest.raises(ValueError, match="optimum: constraints must be a uavhip.solve.Constraints"):
        s.optimum(num_scenes=S, constraints=(None, None, None))
    with pytest.raises(ValueError, match="constraints.capacity: need"):
        s.optimum(num_scenes=S, constraints=Constraints(capacity=torch.ones(S + 1, M, dtype=torch.int32)))
    with pytest.raises(ValueError, match="optimum: N=17 > 16"):
        AllocationSolver(_OnGpu(), 17, M).optimum(num_scenes=S)
    assert s.env is None


class _StubSolver:
    """AllocationSolver for the command line's arithmetic: fixed J per call, no device."""
    calls = []

    def __init__(self, policy, N, M, samples=1):
        self.N, self.M = N, M

    def _alloc(self, J, decoded=None, stats=6):
        import torch

        from uavhip.solve import Allocation
        S = len(J)
        z = torch.zeros(S, dtype=torch.int32)
        return Allocation(torch.full((S, self.N), -1, dtype=torch.int32), torch.tensor(J, dtype=torch.float64), z, z,
                          z.clone(), torch.zeros(S, 1, dtype=torch.float64),
                          decoded_J=None if decoded is None else torch.tensor(decoded, dtype=torch.float64),
                          refine_stats=torch.zeros(S, stats, dtype=torch.int32))

    def solve(self, num_scenes, seed, refine=0, exchanges=0):
        return self._alloc([1.0, 2.0, 3.0, 2.0], [0.5, 1.0, 1.5, 1.0] if refine else None)

    def baseline(self, num_scenes, seed, exchanges=0):
        return self._alloc([2.0, 3.0, 3.0, 2.0] if exchanges else [2.0, 2.0, 3.0, 1.0])

    def optimum(self, num_scenes, seed):
        _StubSolver.calls.append((num_scenes, seed))
        return self._alloc([2.0, 4.0, 3.0, 2.0], stats=2)


def test_command_line_optimum_keys(monkeypatch, capsys):
    """--optimum adds exactly the named keys (and --baseline's), its absence none; N > 16 is refused
    before the device is asked for."""
    import torch

    import uavhip.checkpoint
    import uavhip.policy
    from uavhip import solve

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    with pytest.raises(SystemExit):
        solve.main(["--checkpoint", "x", "--uavs", "17", "--optimum"])
    assert "--uavs <= 16" in capsys.readouterr().err

    class Net:
        def to(self, dev):
            return self
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(uavhip.policy, "TransformerActorCritic", Net)
    monkeypatch.setattr(uavhip.checkpoint, "load_checkpoint", lambda policy, path: None)
    monkeypatch.setattr(solve, "AllocationSolver", _StubSolver)
    argv = ["--checkpoint", "x", "--scenes", "4", "--uavs", "4", "--targets", "4"]

    def run(extra):
        solve.main(argv + extra)
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    for extra in ([], ["--baseline"], ["--refine", "4", "--baseline", "--exchanges", "2"]):
        plain = run(extra)
        assert not [k for k in plain if "optimal" in k], plain
        with_opt = run(extra + ["--optimum"])
        new = [k for k in with_opt if k not in plain]
        want = ["mean_J_optimal", "baseline_over_optimal", "decoded_over_optimal"]
        if "--baseline" not in extra:
            want = ["mean_J_baseline", "policy_beats_baseline"] + want  # --optimum implies --baseline
        if "--refine" in extra:
            want.append("refined_over_optimal")
        want.append("baseline_is_optimal")
        if "--exchanges" in extra:
            want += ["baseline_exchange_over_optimal", "baseline_exchange_is_optimal"]
        assert new == want, (extra, new)
        assert all(with_opt[k] == plain[k] for k in plain if k != "scenes_per_s")
        assert with_opt["mean_J_optimal"] == 2.75 and with_opt["baseline_over_optimal"] == 2.0 / 2.75
        assert with_opt["baseline_is_optimal"] == 0.5
        if "--refine" in extra:
            assert with_opt["decoded_over_optimal"] == 1.0 / 2.75 and with_opt["refined_over_optimal"] == 2.0 / 2.75
            assert with_opt["baseline_exchange_over_optimal"] == 2.5 / 2.75
            assert with_opt["baseline_exchange_is_optimal"] == 0.75
        else:
            assert with_opt["decoded_over_optimal"] == 2.0 / 2.75
    assert _StubSolver.calls and all(c == (4, 0) for c in _StubSolver.calls)
