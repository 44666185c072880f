"""Host-side checks of uavhip_solve_exact_free and uavhip_neighbourhood_pick (no GPU): exact_free_np,
the rule of include/uavhip.h in numpy -- the free list, q_fix and the capacity the held UAVs leave, then
the subset DP over the free-list bits (exact_np of tests/test_exact_host.py on the reduced scene: the free
UAVs' rows of P, the values v q_fix) -- which tests/test_gpu_exact_free.py compares the kernels' J against;
checked here against the plain enumeration of the (M + 1)^K neighbourhood and against exact_np on the FULL
scene with the held UAVs fixed. pick_np, the pick rule restated with tests/device_rng.py's Philox, and its
properties; lns_np, the host loop of the two; and the argument checks of the entry points, of the Python
layers above them and of the command line."""
import ctypes
import itertools
import json

import numpy as np
import pytest

import capi_host
import device_rng
from test_constrained_search_host import check_guarantees, random_constraints
from test_exact_host import _OnGpu, _P, _StubSolver, constraint_cases, convert_ids, exact_np
from test_refine_host import OMEGAS, RTOL_J, J_of, _env_desc, random_starts
from test_search_host import _HostEnv, oracle_tables

_entry_point = capi_host._entry_point("uavhip_solve_exact_free")

NBH_UAV, NBH_TGT = 0x4E424855, 0x4E424854  # the fourth counter word of the UAV keys / the target keys
RANDOM, TARGETS = 0, 1
HELD_SEED = 23


def free_list(N, fixed, max_free):
    """-> (the UAVs in the DP: the first max_free with fixed == 0, ascending; held [N] bool; the free
    UAVs held by overflow)."""
    free = [u for u in range(N) if fixed is None or not fixed[u]]
    dp = free[:max_free]
    held = np.ones(N, bool)
    held[dp] = False
    return dp, held, len(free) - len(dp)


def exact_free_np(p_dmg, p_pen, value, cost, tgt_id, omega, max_free, start=None, allowed=None, fixed=None,
                  capacity=None):
    """uavhip_solve_exact_free for one scene. Scene arguments, start, allowed [N, M], fixed [N], capacity
    [M] as exact_np. -> (assignment [N] int32 target ids, J of that assignment scored with J_of, stats [4]:
    invalid ids, conflicts of the held UAVs, free UAVs in the DP, free UAVs held by overflow)."""
    N, M = np.shape(p_dmg)
    P, v, c, omega = _P(p_dmg, p_pen), np.asarray(value, np.float64), np.asarray(cost, np.float64), float(omega)
    ids, a = convert_ids(tgt_id, start, N)
    invalid = 0 if start is None else sum(1 for w in start if int(w) != -1 and int(w) not in ids)
    dp, held, overflow = free_list(N, fixed, max_free)
    cap = [2 ** 31 - 1] * M if capacity is None else [max(0, int(x)) for x in capacity]
    # pass 1 of the constrained search over the held UAVs, ascending u; q_fix from 1.0 in the same order
    n, conflicts, q_fix = [0] * M, 0, np.ones(M)
    for u in range(N):
        if held[u] and a[u] >= 0:
            conflicts += int(allowed is not None and not allowed[u][a[u]]) + int(n[a[u]] >= cap[a[u]])
            n[a[u]] += 1
            q_fix[a[u]] = q_fix[a[u]] * (1.0 - P[u][a[u]])
    out = [a[u] if held[u] else -1 for u in range(N)]
    if dp:
        left = None if capacity is None else np.array([max(cap[t], n[t]) - n[t] for t in range(M)], np.int32)
        sub, _ = exact_np(P[dp], np.ones(len(dp)), v * q_fix, c[dp], np.arange(M), omega, None,
                          None if allowed is None else np.asarray(allowed)[dp], None, left)
        for b, u in enumerate(dp):
            out[u] = int(sub[b])
    return (np.array([ids[t] if t >= 0 else -1 for t in out], np.int32), J_of(P, v, c, omega, out),
            np.array([invalid, conflicts, len(dp), overflow], np.int32))


def enumerate_free_np(p_dmg, p_pen, value, cost, tgt_id, omega, max_free, start=None, allowed=None, fixed=None,
                      capacity=None):
    """Plain enumeration of the neighbourhood: the largest J (J_of) over every placement of the UAVs in
    the DP on {none, 0..M-1} that the header admits, the held UAVs where the start puts them.
    -> (J, the number of feasible placements)."""
    N, M = np.shape(p_dmg)
    P, v, c = _P(p_dmg, p_pen), np.asarray(value, np.float64), np.asarray(cost, np.float64)
    _, a = convert_ids(tgt_id, start, N)
    dp, held, _ = free_list(N, fixed, max_free)
    n_held = [sum(1 for u in range(N) if held[u] and a[u] == t) for t in range(M)]
    best, count = -np.inf, 0
    for place in itertools.product(range(-1, M), repeat=len(dp)):
        if allowed is not None and any(t >= 0 and not allowed[u][t] for u, t in zip(dp, place)):
            continue
        if capacity is not None and any(n_held[t] + place.count(t) > max(max(0, int(capacity[t])), n_held[t])
                                        for t in set(place) if t >= 0):
            continue
        x = [a[u] if held[u] else -1 for u in range(N)]
        for u, t in zip(dp, place):
            x[u] = t
        best, count = max(best, J_of(P, v, c, float(omega), x)), count + 1
    return best, count


def held_case(case, N, M, E, p_held=0.4, seed=HELD_SEED):
    """A constraint case of test_exact_host.constraint_cases merged with a random held set: (start [E, N]
    ids -- the case's fixed ids over random ones --, allowed, fixed [E, N] uint8 = the case's | the held
    set, capacity)."""
    _, start, allowed, fixed, capacity = case
    rng = np.random.default_rng(seed)
    base = random_starts(N, M, E, seed)
    if start is not None and fixed is not None:
        base = np.where(fixed != 0, start, base).astype(np.int32)
    more = (rng.random((E, N)) < p_held).astype(np.uint8)
    return base, allowed, more if fixed is None else (more | (fixed != 0)).astype(np.uint8), capacity


def exact_free_rows(p_dmg, p_pen, value, cost, tgt_id, omega, max_free, starts=None, allowed=None, fixed=None,
                    capacity=None):
    """exact_free_np over rows -> (assignment [S, N], J [S], stats [S, 4])."""
    pick = lambda x, s: None if x is None else x[s]  # noqa: E731
    rows = [exact_free_np(p_dmg[s], p_pen[s], value[s], cost[s], tgt_id[s], omega, max_free, pick(starts, s),
                          pick(allowed, s), pick(fixed, s), pick(capacity, s)) for s in range(len(p_dmg))]
    return tuple(np.array([r[i] for r in rows]) for i in range(3))


# ---------------------------------------------------------------------------------- the pick rule
def pick_keys(n, round, s, seed, stream):
    """Key i < n: word i & 3 of philox4x32_10({i >> 2, round, s, stream}, the seed's two halves)."""
    i = np.arange(n)
    words = device_rng.philox_v((i >> 2, round, s, stream), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [int(words[k & 3][k]) for k in range(n)]


def pick_np(N, M, K, mode, round, seed, s, a=None, fixed_in=None):
    """uavhip_neighbourhood_pick for row s: a [N] LIST indices or -1 (None: all idle), fixed_in [N] or
    None -> fixed_out [N] uint8, 1 = held."""
    ku = pick_keys(N, round, s, seed, NBH_UAV)
    g = [0] * N
    if mode == TARGETS and a is not None:
        kt = pick_keys(M, round, s, seed, NBH_TGT)
        order = sorted(range(M), key=lambda t: (kt[t], t))
        rank = {t: r for r, t in enumerate(order)}
        g = [0 if a[u] < 0 else 1 + rank[int(a[u])] for u in range(N)]
    open_ = [u for u in range(N) if fixed_in is None or not fixed_in[u]]
    out = np.ones(N, np.uint8)
    out[sorted(open_, key=lambda u: (g[u], ku[u], u))[:K]] = 0
    return out


def lns_np(p_dmg, p_pen, value, cost, tgt_id, omega, s, start, rounds, K, mode, seed, allowed=None, fixed=None,
           capacity=None):
    """VecUAVEnv.lns_assignments for row s on the host: rounds of pick_np + exact_free_np, the new result
    kept where its J is strictly greater. -> (assignment ids, J, the J after every round)."""
    N, M = np.shape(p_dmg)
    P, v, c = _P(p_dmg, p_pen), np.asarray(value, np.float64), np.asarray(cost, np.float64)
    ids, a = convert_ids(tgt_id, start, N)
    best = np.array([ids[t] if t >= 0 else -1 for t in a], np.int32)
    J, trace = J_of(P, v, c, float(omega), a), []
    for r in range(rounds):
        held = pick_np(N, M, K, mode, r, seed, s, convert_ids(tgt_id, best, N)[1], fixed)
        new, Jn, _ = exact_free_np(p_dmg, p_pen, value, cost, tgt_id, omega, K, best, allowed, held, capacity)
        if Jn > J:
            best, J = new, Jn
        trace.append(J)
    return best, J, trace


# ---------------------------------------------------------------------------------- exact_free_np
@pytest.mark.parametrize("N,M,K,E", [(6, 4, 3, 3), (7, 5, 4, 2)])
def test_exact_free_np_is_the_enumeration(N, M, K, E):
    """Every placement of the K UAVs in the DP enumerated ((M + 1)^K = 125 and 1296), under every
    constraint case merged with a held set: the restatement's J is the enumeration's maximum to the reward
    bar, its assignment keeps the guarantees, and the held UAVs leave as they came."""
    for omega in OMEGAS:
        tabs = oracle_tables(N, M, E, omega)
        for case in constraint_cases(N, M, E):
            start, allowed, fixed, capacity = held_case(case, N, M, E)
            pick = lambda x, s: None if x is None else x[s]  # noqa: E731
            n_over = 0
            for s in range(E):
                args = tuple(t[s] for t in tabs) + (omega, K, start[s], pick(allowed, s), fixed[s], pick(capacity, s))
                asg, J, st = exact_free_np(*args)
                Jb, n = enumerate_free_np(*args)
                assert abs(J - Jb) <= RTOL_J * max(1.0, abs(Jb)), (case[0], omega, s, J, Jb)
                dp, held, overflow = free_list(N, fixed[s], K)
                assert n <= (M + 1) ** len(dp) and list(st[2:]) == [len(dp), overflow]
                n_over += overflow
                check_guarantees((case[0], omega, s), asg[None], tabs[4][s][None], start[s][None],
                                 pick(allowed, s)[None] if allowed is not None else None, held.astype(np.uint8)[None],
                                 pick(capacity, s)[None] if capacity is not None else None)
            print(f"({N}, {M}, K = {K}) omega {omega} {case[0]}: {n_over} free UAVs held by overflow")


@pytest.mark.parametrize("N,M,E,K", [(5, 7, 3, 3), (9, 12, 2, 6), (12, 6, 2, 12)])
def test_exact_free_np_is_exact_np_with_the_held_uavs_fixed(N, M, E, K):
    """The same problem put to exact_np on the FULL scene -- every held UAV, overflow included, a fixed
    one -- gives the same J to the reward bar: q_fix and the capacity left restate what `must` sets do."""
    for omega in OMEGAS:
        tabs = oracle_tables(N, M, E, omega)
        for case in constraint_cases(N, M, E):
            start, allowed, fixed, capacity = held_case(case, N, M, E)
            if K == N:
                fixed = None if case[3] is None else case[3]  # all free but the case's own: the whole table
            pick = lambda x, s: None if x is None else x[s]  # noqa: E731
            for s in range(E):
                rest = (start[s], pick(allowed, s))
                _, J, st = exact_free_np(*(t[s] for t in tabs), omega, K, *rest, pick(fixed, s), pick(capacity, s))
                held = free_list(N, pick(fixed, s), K)[1].astype(np.uint8)
                _, Jx = exact_np(*(t[s] for t in tabs), omega, *rest, held, pick(capacity, s))
                assert abs(J - Jx) <= RTOL_J * max(1.0, abs(Jx)), (case[0], omega, s, J, Jx)
                # never below the start where the start is feasible for the held problem: all UAVs held
                _, J0, _ = exact_free_np(*(t[s] for t in tabs), omega, K, *rest, np.ones(N, np.uint8), pick(capacity, s))
                if allowed is None and capacity is None:
                    assert J >= J0 - RTOL_J * max(1.0, abs(J0)), (case[0], omega, s, J, J0)


def test_all_free_is_exact_np():
    """fixed = None and max_free = N: q_fix = 1.0 everywhere and the reduced scene is the scene."""
    N, M, E = 5, 7, 3
    tabs = oracle_tables(N, M, E, 0.5)
    for s in range(E):
        asg, J, st = exact_free_np(*(t[s] for t in tabs), 0.5, N)
        want, Jx = exact_np(*(t[s] for t in tabs), 0.5)
        assert np.array_equal(asg, want) and J == Jx and list(st) == [0, 0, N, 0]


# ---------------------------------------------------------------------------------- pick_np
@pytest.mark.parametrize("N,M", [(5, 7), (16, 32), (33, 34), (64, 128)])
def test_pick_np_properties(N, M):
    """Exactly min(K, open) UAVs are freed; fixed_in is never freed; in TARGETS mode the idle open UAVs
    go first and at most one target's crew is split (the last one taken); rounds, rows and seeds differ."""
    rng = np.random.default_rng(3)
    a = rng.integers(-1, M, N)
    a[rng.random(N) < 0.2] = -1
    for K, with_fixed in itertools.product((1, 3, 12, 16), (False, True)):
        fixed_in = (rng.random(N) < 0.3).astype(np.uint8) if with_fixed else None
        n_open = N if fixed_in is None else int((fixed_in == 0).sum())
        for mode in (RANDOM, TARGETS):
            seen = set()
            for round, s, seed in ((0, 0, 5), (1, 0, 5), (0, 1, 5), (0, 0, 6), (0, 0, 5 + (1 << 32))):
                out = pick_np(N, M, K, mode, round, seed, s, a, fixed_in)
                seen.add(out.tobytes())
                assert int((out == 0).sum()) == min(K, n_open)
                assert fixed_in is None or bool((out[fixed_in != 0] == 1).all())
                if mode == TARGETS:
                    opened = np.array([fixed_in is None or not fixed_in[u] for u in range(N)])
                    idle_held = bool((opened & (a < 0) & (out == 1)).any())
                    assert not (idle_held and bool((opened & (a >= 0) & (out == 0)).any()))
                    split = [t for t in range(M) if len({int(out[u]) for u in range(N) if opened[u] and a[u] == t}) == 2]
                    assert len(split) <= 1, (N, M, K, split)
            assert len(seen) >= (3 if mode == RANDOM and N >= 16 and K < n_open else 1)
    # mode RANDOM does not read the assignment; TARGETS without one is RANDOM's order
    assert np.array_equal(pick_np(N, M, 3, RANDOM, 2, 9, 1, a), pick_np(N, M, 3, RANDOM, 2, 9, 1, None))
    assert np.array_equal(pick_np(N, M, 3, TARGETS, 2, 9, 1, None), pick_np(N, M, 3, RANDOM, 2, 9, 1, None))


def test_pick_keys_are_the_multistart_philox():
    """The keys' generator is the Philox4x32-10 of the multi-start rule: its known answers, and the
    word order (key i is word i & 3 of block i >> 2)."""
    from test_multistart_host import philox4x32_10
    for round, s, seed in ((0, 0, 0), (3, 2, 0x123456789ABCDEF)):
        keys = pick_keys(9, round, s, seed, NBH_UAV)
        for i in range(9):
            assert keys[i] == philox4x32_10((i >> 2, round, s, NBH_UAV), (seed & 0xFFFFFFFF, seed >> 32))[i & 3]
    assert pick_keys(4, 0, 0, 0, NBH_UAV) != pick_keys(4, 0, 0, 0, NBH_TGT)


def test_lns_np_never_decreases():
    """12 x 24, K = 6, 4 rounds from the empty start: J never decreases over the rounds, in the doubles."""
    N, M, E = 12, 24, 2
    tabs = oracle_tables(N, M, E, 0.5)
    for s, mode in itertools.product(range(E), (RANDOM, TARGETS)):
        _, J, trace = lns_np(*(t[s] for t in tabs), 0.5, s, None, 4, 6, mode, 1)
        assert trace == sorted(trace) and J == trace[-1] and trace[0] > 0.0


# ---------------------------------------------------------------------------------- bindings and checks
def test_binding_signatures():
    from uavhip import _lib
    vp, i32, i64, u32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
    res, args = _lib._SIGS["uavhip_solve_exact_free"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), i32, i32, i32] + [vp] * 9 + [i64, vp]
    assert _lib.LIB.uavhip_solve_exact_free.argtypes == args
    assert _lib._SIGS["uavhip_exact_free_workspace_bytes"] == (i64, [i32, i32, i32])
    assert _lib.LIB.uavhip_exact_free_workspace_bytes.restype is i64
    res, args = _lib._SIGS["uavhip_neighbourhood_pick"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), i32, i32, i32, i32, u32, u64, vp, vp, vp, vp]
    assert _lib.LIB.uavhip_neighbourhood_pick.argtypes == args
    assert _lib.LIB.uavhip_abi_version() == 6 and _lib.EXACT_MAX_N == 16 and _lib.EXACT_FREE_MAX == 16
    assert _lib.NBH == dict(random=RANDOM, targets=TARGETS)


def test_workspace_bytes():
    from uavhip import _lib
    need = _lib.LIB.uavhip_exact_free_workspace_bytes
    # two D tables of 2^K doubles, the choice table [M][2^K] of uint16, M 16-byte records, the 16-byte list
    for K, M in ((1, 1), (3, 7), (12, 128), (16, 2), (16, 128)):
        assert need(K, M, 1) == 2 * 8 * 2 ** K + ((M * 2 * 2 ** K + 15) & ~15) + 16 * M + 16, (K, M)
        assert need(K, M, 5) == 5 * need(K, M, 1) and need(K, M, 1) % 16 == 0
    for bad in ((0, 4, 1), (17, 4, 1), (4, 0, 1), (4, 129, 1), (4, 4, 0), (-1, 4, 1), (4, 4, -3)):
        assert need(*bad) == -1, bad


def test_argument_checks_without_gpu():
    """Every documented misuse of the two entry points returns UAVHIP_EINVAL with a message naming the
    function, before any HIP call (the placeholders would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_solve_exact_free, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_solve_exact_free"
    row = int(_lib.LIB.uavhip_exact_free_workspace_bytes(5, 4, 1))

    def call(env=None, stride=1, S=6, K=5, allowed=P, fixed=P, cap=P, ain=P, out=P, J=P, cov=P, stats=P, ws=P, nbytes=row):
        return fn(env or _env_desc(), stride, S, K, allowed, fixed, cap, ain, out, J, cov, stats, ws, nbytes, None)

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
    for K in (0, -1, 17):
        assert call(K=K, nbytes=1 << 40) == -1 and name in err() and f"max_free={K}".encode() in err()
    assert call(ain=None) == -1 and name in err() and b"fixed without assignment_in" in err()
    assert call(nbytes=row - 1) == -1 and name in err() and b"workspace" in err()   # one byte short of a row
    # more bits than UAVs count as N of them: a row of N = 8 bits is enough for max_free = 16, one byte less is not
    row8 = int(_lib.LIB.uavhip_exact_free_workspace_bytes(8, 4, 1))
    assert call(K=16, nbytes=row8 - 1) == -1 and name in err() and b"workspace" in err()
    big = int(_lib.LIB.uavhip_exact_free_workspace_bytes(16, 128, 1))
    assert call(env=_env_desc(N=64, M=128), K=16, nbytes=big - 1) == -1 and name in err() and b"workspace" in err()
    assert call(nbytes=0) == -1 and name in err() and b"workspace" in err()
    assert call(nbytes=-5) == -1 and name in err() and b"workspace" in err()
    assert call(ws=None) == -1 and name in err() and b"workspace" in err()
    assert call(ws=ctypes.c_void_p(24)) == -1 and name in err() and b"aligned" in err()
    assert call(allowed=None, fixed=None, cap=None, ain=None, out=None) == -1 and name in err()
    assert fn(None, 1, 1, 5, P, P, P, P, P, P, P, P, P, row, None) == -1 and name in err()

    fn, name = _lib.LIB.uavhip_neighbourhood_pick, b"uavhip_neighbourhood_pick"

    def pick(env=None, stride=1, S=6, K=5, mode=TARGETS, round=0, seed=1, asg=P, fixed_in=P, out=P):
        return fn(env or _env_desc(), stride, S, K, mode, round, seed, asg, fixed_in, out, None)

    assert pick(out=None) == -1 and name in err() and b"fixed_out non-NULL" in err()
    assert pick(stride=0) == -1 and name in err() and b"env_stride=0" in err()
    assert pick(S=0) == -1 and name in err() and b"S=0" in err()
    assert pick(S=7) == -1 and name in err() and b"E=6" in err()
    assert pick(stride=3, S=3) == -1 and name in err() and b"E=6" in err()
    assert pick(stride=1 << 30, S=1 << 30) == -1 and name in err()
    for K in (0, -1, 17):
        assert pick(K=K) == -1 and name in err() and f"K={K}".encode() in err()
    for mode in (-1, 2):
        assert pick(mode=mode) == -1 and name in err() and f"mode={mode}".encode() in err()
    assert pick(env=_env_desc(N=65)) == -1 and name in err() and b"bad env dims" in err()
    assert fn(None, 1, 1, 5, 0, 0, 0, P, P, P, None) == -1 and name in err()


def test_python_layers_refuse_before_any_device_call():
    import torch

    from uavhip import AllocationSolver
    from uavhip.vec_env import VecUAVEnv
    E, N, M = 6, 4, 4
    env = _HostEnv(E, N, M)
    asg = torch.zeros(E, N, dtype=torch.int32)
    call = lambda *a, **k: VecUAVEnv.exact_free_assignments(env, *a, **k)  # noqa: E731
    with pytest.raises(TypeError, match="max_free"):
        call()
    with pytest.raises(ValueError, match="exact_free_assignments: stride=0"):
        call(max_free=3, stride=0)
    with pytest.raises(ValueError, match="exact_free_assignments: rows=7"):
        call(max_free=3, rows=7)
    with pytest.raises(ValueError, match="exact_free_assignments: rows=3 at stride=3"):
        call(max_free=3, stride=3, rows=3)
    for K in (0, -1, 17):
        with pytest.raises(ValueError, match=f"exact_free_assignments: max_free={K} must be in"):
            call(max_free=K)
    with pytest.raises(ValueError, match="exact_free_assignments: fixed needs assignment"):
        call(max_free=3, fixed=torch.zeros(E, N, dtype=torch.uint8))
    with pytest.raises(ValueError, match="assignment: need a contiguous torch.int32"):
        call(torch.zeros(E, N, dtype=torch.int64), max_free=3)
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8 tensor of 48"):
        call(max_free=3, allowed=torch.ones(E, N, M, dtype=torch.uint8), stride=2)  # row-indexed: 3 rows at stride 2
    with pytest.raises(ValueError, match="fixed: need a contiguous torch.uint8"):
        call(asg, max_free=3, fixed=torch.zeros(E, N + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="capacity: need a contiguous torch.int32"):
        call(max_free=3, capacity=torch.zeros(E, M, dtype=torch.int64))
    with pytest.raises(ValueError, match="stats: need a contiguous torch.int32"):
        call(max_free=3, stats=torch.zeros(E, 2, dtype=torch.int32))  # exact_assignments' shape
    with pytest.raises(ValueError, match="J: need a contiguous torch.float64"):
        call(max_free=3, J=torch.zeros(E, dtype=torch.float32))
    with pytest.raises(ValueError, match="max_workspace_bytes=100 holds no row"):
        call(max_free=3, max_workspace_bytes=100)

    pick = lambda *a, **k: VecUAVEnv.pick_neighbourhood(env, *a, **k)  # noqa: E731
    with pytest.raises(ValueError, match="pick_neighbourhood: stride=0"):
        pick(asg, 3, "targets", 0, 0, stride=0)
    with pytest.raises(ValueError, match="pick_neighbourhood: rows=7"):
        pick(asg, 3, "targets", 0, 0, rows=7)
    for K in (0, 17):
        with pytest.raises(ValueError, match=f"pick_neighbourhood: K={K} must be in"):
            pick(asg, K, "targets", 0, 0)
    for mode in ("crews", 1, None):
        with pytest.raises(ValueError, match="pick_neighbourhood: mode must be one of"):
            pick(asg, 3, mode, 0, 0)
    for round in (-1, 1 << 32):
        with pytest.raises(ValueError, match="pick_neighbourhood: round="):
            pick(asg, 3, "random", round, 0)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="pick_neighbourhood: seed="):
            pick(asg, 3, "random", 0, seed)
    with pytest.raises(ValueError, match="assignment: need a contiguous torch.int32"):
        pick(asg.long(), 3, "random", 0, 0)
    with pytest.raises(ValueError, match="fixed: need a contiguous torch.uint8"):
        pick(asg, 3, "random", 0, 0, fixed=torch.zeros(E, N, dtype=torch.bool))
    with pytest.raises(ValueError, match="out: need a contiguous torch.uint8"):
        pick(asg, 3, "random", 0, 0, out=torch.zeros(E, N, dtype=torch.int32))

    lns = lambda *a, **k: VecUAVEnv.lns_assignments(env, *a, **k)  # noqa: E731
    with pytest.raises(ValueError, match="lns_assignments: rounds=-1 must be >= 0"):
        lns(asg, rounds=-1, free=3)
    for K in (0, 17):
        with pytest.raises(ValueError, match=f"lns_assignments: free={K} must be in"):
            lns(asg, rounds=2, free=K)
    with pytest.raises(ValueError, match="lns_assignments: mode must be one of"):
        lns(asg, rounds=2, free=3, mode="crews")
    with pytest.raises(ValueError, match="lns_assignments: seed=-1"):
        lns(asg, rounds=2, free=3, seed=-1)
    with pytest.raises(ValueError, match="lns_assignments: assignment is required"):
        lns(None, rounds=2, free=3)
    with pytest.raises(ValueError, match="lns_assignments: rows=7"):
        lns(asg, rounds=2, free=3, rows=7)
    with pytest.raises(ValueError, match="capacity: need a contiguous torch.int32"):
        lns(asg, rounds=2, free=3, capacity=torch.zeros(E, M, dtype=torch.int64))

    s = AllocationSolver(_OnGpu(), N, M, samples=2)
    for what in (s.solve, s.baseline):
        with pytest.raises(ValueError, match=f"{what.__name__}: lns_rounds must be >= 0"):
            what(num_scenes=2, lns_rounds=-1)
        for K in (0, 17):
            with pytest.raises(ValueError, match=f"{what.__name__}: lns_free={K} must be in"):
                what(num_scenes=2, lns_rounds=2, lns_free=K)
        with pytest.raises(ValueError, match=f"{what.__name__}: lns_mode must be one of"):
            what(num_scenes=2, lns_rounds=2, lns_mode="crews")
    assert s.env is None


class _LnsStub(_StubSolver):
    """_StubSolver with baseline(lns_rounds=): the arguments are recorded."""
    seen = []

    def baseline(self, num_scenes, seed, exchanges=0, restarts=0, lns_rounds=0, lns_free=12, lns_mode="targets"):
        import dataclasses

        import torch
        if lns_rounds:
            _LnsStub.seen.append((exchanges, lns_rounds, lns_free, lns_mode))
            return dataclasses.replace(self._alloc([2.0, 4.0, 3.0, 1.5]),
                                       lns_J_before=torch.tensor([2.0, 3.0, 3.0, 1.0], dtype=torch.float64))
        if restarts:
            return self._alloc([2.0, 4.0, 3.0, 1.0], stats=10)
        return super().baseline(num_scenes, seed, exchanges)


def test_command_line_lns_keys(monkeypatch, capsys):
    """--lns adds exactly the named keys (and --baseline's), its absence none; the start is the baseline
    at --exchanges' cap or 32; values out of range are refused before the device is asked for."""
    import torch

    import uavhip.checkpoint
    import uavhip.policy
    from uavhip import solve

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    for bad, msg in ((["--lns", "-1"], "--lns must be >= 0"), (["--lns", "2", "--lns-free", "17"], "--lns-free must be in"),
                     (["--lns", "2", "--lns-free", "0"], "--lns-free must be in"),
                     (["--lns", "2", "--lns-mode", "crews"], "--lns-mode")):
        with pytest.raises(SystemExit):
            solve.main(["--checkpoint", "x"] + bad)
        assert msg in capsys.readouterr().err

    class Net:
        def to(self, dev):
            return self
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(uavhip.policy, "TransformerActorCritic", Net)
    monkeypatch.setattr(uavhip.checkpoint, "load_checkpoint", lambda policy, path: None)
    monkeypatch.setattr(solve, "AllocationSolver", _LnsStub)
    argv = ["--checkpoint", "x", "--scenes", "4", "--uavs", "4", "--targets", "4"]

    def run(extra):
        solve.main(argv + extra)
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    for extra in ([], ["--baseline"], ["--optimum"], ["--restarts", "4"],
                  ["--refine", "4", "--baseline", "--exchanges", "2", "--optimum"]):
        plain = run(extra)
        assert not [k for k in plain if "lns" in k], plain
        _LnsStub.seen.clear()
        with_lns = run(extra + ["--lns", "3", "--lns-free", "5", "--lns-mode", "random"])
        new = [k for k in with_lns if k not in plain]
        want = ["mean_J_lns", "lns_improved"]
        if not {"--baseline", "--optimum", "--restarts"} & set(extra):
            want = ["mean_J_baseline", "policy_beats_baseline"] + want  # --lns implies --baseline
        if "--optimum" in extra:
            want += ["lns_over_optimal", "lns_is_optimal"]
        assert new == want, (extra, new)
        assert [k for k in with_lns if k in plain] == list(plain)  # the existing keys keep their order
        assert all(with_lns[k] == plain[k] for k in plain if k != "scenes_per_s")
        assert with_lns["mean_J_lns"] == 2.625 and with_lns["lns_improved"] == 0.5
        assert _LnsStub.seen == [(2 if "--exchanges" in extra else 32, 3, 5, "random")]
        if "--optimum" in extra:
            assert with_lns["lns_over_optimal"] == 2.625 / 2.75 and with_lns["lns_is_optimal"] == 0.75
