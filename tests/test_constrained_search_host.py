"""Host-side checks of uavhip_search_assignments_constrained (no GPU): constrained_search_np, the
restatement of the constrained rule (include/uavhip.h) in Python floats that
tests/test_gpu_constrained_search.py compares the kernel against bit for bit -- the arithmetic of its
sweeps and its scan is refine_np's and best_exchange's (tests/test_refine_host.py,
tests/test_search_host.py), and without constraints it is search_np exactly; its feasibility and local
optimality within the constraints on scenes small enough to enumerate; the cases the GPU tests run;
and the argument checks of the entry point and of the Python layers above it."""
import ctypes
import itertools

import numpy as np
import pytest

import capi_host
from test_refine_host import OMEGAS, RTOL_J, J_of, _env_desc, host_scenes, prm, random_starts, refine_np
from test_search_host import CAPS, SHAPES, _HostEnv, oracle_tables, search_np

# (N, M, E) of the conditions below; the GPU test adds (17, 20, 5), (33, 34, 3), (34, 66, 2) and (8, 128, 3)
CASE_SHAPES = [(5, 7, 33), (16, 32, 32), (12, 70, 5)]
EITHER = (8, 128, 3)
DENSITY, CAP_CHOICES, P_FIXED = 0.7, (1, 2, 3), 0.2
CONSTRAINT_SEED = 11


_entry_point = capi_host._entry_point("uavhip_search_assignments_constrained")


def random_constraints(N, M, E, seed=CONSTRAINT_SEED):
    """Seeded constraints in the entry point's layout: allowed [E, N, M] uint8 of density 0.7,
    capacity [E, M] int32 uniform in {1, 2, 3}, fixed_ids [E, N] int32: each UAV with probability 0.2
    committed to a uniform target id of [0, M) or to none (-1), else free (-2)."""
    rng = np.random.default_rng(seed)
    allowed = (rng.random((E, N, M)) < DENSITY).astype(np.uint8)
    capacity = rng.choice(CAP_CHOICES, (E, M)).astype(np.int32)
    fixed_ids = rng.integers(-1, M, (E, N)).astype(np.int32)
    fixed_ids[rng.random((E, N)) >= P_FIXED] = -2
    return allowed, capacity, fixed_ids


def with_fixed(start, fixed_ids):
    """(start [E, N] with the committed UAVs' ids written in -- None: the empty start --, fixed [E, N] uint8)."""
    base = np.full(fixed_ids.shape, -1, np.int32) if start is None else start
    return np.where(fixed_ids != -2, fixed_ids, base).astype(np.int32), (fixed_ids != -2).astype(np.uint8)


def neutral_constraints(N, M, E):
    return np.ones((E, N, M), np.uint8), np.zeros((E, N), np.uint8), np.full((E, M), N, np.int32)


def constrained_search_np(p_dmg, p_pen, value, cost, tgt_id, omega, start=None, allowed=None, fixed=None,
                          capacity=None, max_exchanges=32, max_sweeps=32):
    """uavhip_search_assignments_constrained for one scene, in Python floats. Scene arguments and
    start as refine_np; allowed [N, M], fixed [N], capacity [M] or None.
    -> (assignment [N] int32 target ids, J, covered, stats [8] int32 = sweeps, moves, phase_converged,
    invalid ids, exchanges, scan_clean, dropped, fixed_conflicts; J after every phase (list))."""
    N, M = np.shape(p_dmg)
    P = [[float(p_dmg[u][t]) * float(p_pen[u]) for t in range(M)] for u in range(N)]
    v, omega = [float(x) for x in value], float(omega)
    wc = [omega * float(x) for x in cost]
    ids = [int(x) for x in tgt_id]
    ok = [[True] * M for _ in range(N)] if allowed is None else [[bool(allowed[u][t]) for t in range(M)] for u in range(N)]
    fx = [False] * N if fixed is None else [bool(x) for x in fixed]
    cap = [2 ** 31 - 1] * M if capacity is None else [max(0, int(x)) for x in capacity]
    a, invalid = [-1] * N, 0
    if start is not None:
        for u in range(N):
            want = int(start[u])
            if want == -1:
                continue
            if want in ids:
                a[u] = ids.index(want)
            else:
                invalid += 1
    # the start: pass 1 over the fixed UAVs, pass 2 over the free ones, each in ascending u
    n, dropped, conflicts = [0] * M, 0, 0
    for u in range(N):
        if fx[u] and a[u] >= 0:
            conflicts += int(not ok[u][a[u]]) + int(n[a[u]] >= cap[a[u]])
            n[a[u]] += 1
    for u in range(N):
        if not fx[u] and a[u] >= 0:
            if not ok[u][a[u]] or n[a[u]] >= cap[a[u]]:
                a[u] = -1
                dropped += 1
            else:
                n[a[u]] += 1

    def products(skip):
        Q, cnt = [1.0] * M, [0] * M
        for w in range(N):
            if w != skip and a[w] >= 0:
                Q[a[w]] = Q[a[w]] * (1.0 - P[w][a[w]])
                cnt[a[w]] += 1
        return Q, cnt

    def g(u, x, Q):
        return 0.0 if x < 0 else (v[x] * Q) * P[u][x] - wc[u]

    def scan():
        Qo = [products(u)[0][a[u]] if a[u] >= 0 else 1.0 for u in range(N)]
        best = None
        for i in range(N):
            for j in range(i + 1, N):
                s, t = a[i], a[j]
                if fx[i] or fx[j] or s == t or (s >= 0 and not ok[j][s]) or (t >= 0 and not ok[i][t]):
                    continue
                d = (g(j, s, Qo[i]) + g(i, t, Qo[j])) - (g(i, s, Qo[i]) + g(j, t, Qo[j]))
                if best is None or d > best[0]:
                    best = (d, i, j)
        return best

    def score():
        """J and covered of a: refine_np's own, from a scored without a sweep."""
        _, J, cov, _, _, _ = refine_np(p_dmg, p_pen, value, cost, range(M), omega, a, 0)
        return J, cov

    sweeps = moves = x = 0
    trace = []
    while True:
        last, converged = sweeps + max_sweeps, 1
        while sweeps < last:
            moved = False
            for u in range(N):
                if fx[u]:
                    continue
                Q, cnt = products(u)
                gains = [g(u, t, Q[t]) for t in range(M)]
                cur = gains[a[u]] if a[u] >= 0 else 0.0
                cand, gain = -1, 0.0
                for t in range(M):
                    if ok[u][t] and (t == a[u] or cnt[t] < cap[t]) and gains[t] > gain:
                        cand, gain = t, gains[t]
                if gain > cur:
                    a[u] = cand
                    moved = True
                    moves += 1
            sweeps += 1
            converged = int(not moved)
            if not moved:
                break
        J, cov = score()
        trace.append(J)
        if max_exchanges == 0:
            clean = 0
            break
        best = scan()
        if best is None or not best[0] > 0.0:
            clean = 1
            break
        if x == max_exchanges:
            clean = 0
            break
        _, i, j = best
        a[i], a[j] = a[j], a[i]
        x += 1
    out = np.array([ids[t] if t >= 0 else -1 for t in a], np.int32)
    return out, J, cov, np.array([sweeps, moves, converged, invalid, x, clean, dropped, conflicts], np.int32), trace


def constrained_rows(p_dmg, p_pen, value, cost, tgt_id, omega, starts, allowed, fixed, capacity, max_exchanges=32,
                     max_sweeps=32):
    """constrained_search_np over rows: (assignment [S, N], J [S], covered [S], stats [S, 8], traces)."""
    pick = lambda x, s: None if x is None else x[s]  # noqa: E731
    rows = [constrained_search_np(p_dmg[s], p_pen[s], value[s], cost[s], tgt_id[s], omega, pick(starts, s),
                                  pick(allowed, s), pick(fixed, s), pick(capacity, s), max_exchanges, max_sweeps)
            for s in range(len(p_dmg))]
    return tuple(np.array([r[i] for r in rows]) for i in range(4)) + ([r[4] for r in rows],)


def list_indices(asg, tgt_id):
    """[S, N] target ids -> list indices (-1 kept): the lowest list index of an id."""
    out = np.full(asg.shape, -1, np.int64)
    for s in range(len(asg)):
        ids = [int(i) for i in tgt_id[s]]
        out[s] = [ids.index(int(i)) if i >= 0 else -1 for i in asg[s]]
    return out


def check_guarantees(label, asg, tgt_id, start, allowed, fixed, capacity):
    """The guarantees of the header on the outputs themselves: a free UAV's pair is allowed, no target
    holds more UAVs than max(capacity, its fixed UAVs), a fixed UAV leaves as it came (an id that
    matches no target as -1). None arrays constrain nothing."""
    S, N = asg.shape
    a = list_indices(asg, tgt_id)
    for s in range(S):
        fx = np.zeros(N, bool) if fixed is None else fixed[s].astype(bool)
        for u in range(N):
            if fx[u]:
                came = -1 if start is None else int(start[s][u])
                assert int(asg[s][u]) == (came if came in [int(i) for i in tgt_id[s]] else -1), (label, s, u)
            elif a[s][u] >= 0 and allowed is not None:
                assert allowed[s][u][a[s][u]], (label, s, u)
        if capacity is not None:
            for t in range(capacity.shape[1]):
                on = a[s] == t
                assert on.sum() <= max(max(0, int(capacity[s][t])), int((on & fx).sum())), (label, s, t)


def check_constrained_conditions(label, empty, rand, tgt_id, capacity, want=True):
    """The conditions of a case (one shape at one omega; empty / rand = constrained_rows results from
    the empty start and from random ids) at caps 32 / 32: every row ends converged with a clean scan,
    and (want) some row ends with a target that holds >= 2 UAVs and is at its capacity, some row makes
    an exchange, and from the random ids some row drops a pair in pass 2."""
    full = 0
    for r in (empty, rand):
        assert bool((r[3][:, 2] == 1).all()) and bool((r[3][:, 5] == 1).all()), label
        assert bool((r[3][:, 4] < CAPS[0]).all()), label
        a = list_indices(r[0], tgt_id)
        for s in range(len(a)):
            n = np.bincount(a[s][a[s] >= 0], minlength=capacity.shape[1])
            full += int(((n >= 2) & (n == capacity[s])).any())
    ex = int((empty[3][:, 4] > 0).sum() + (rand[3][:, 4] > 0).sum())
    dropped = int(rand[3][:, 6].sum())
    print(f"{label}: {full} runs end with a full target of >= 2 UAVs, {ex} exchange, {dropped} pairs dropped from "
          f"random ids, {int(empty[3][:, 7].sum())} fixed conflicts, mean J {empty[1].mean():.6f}")
    if want:
        assert full > 0 and ex > 0 and dropped > 0, label


def test_without_constraints_it_is_search_np():
    """No constraints and neutral ones (all allowed, none fixed, capacity N): assignment, J, covered
    and stats[:6] are search_np's exactly, from the empty and the random starts, with and without
    exchanges; nothing is dropped and nothing conflicts."""
    for (N, M, E), omega in itertools.product(SHAPES, OMEGAS):
        tabs = oracle_tables(N, M, E, omega)
        starts = random_starts(N, M, E)
        starts[0, 0] = M + 3  # an id of no target
        al, fx, cp = neutral_constraints(N, M, E)
        for s in range(E):
            args = tuple(t[s] for t in tabs) + (omega,)
            for start, caps in ((None, CAPS), (starts[s], CAPS), (starts[s], (0, 32)), (starts[s], (2, 1))):
                want = search_np(*args, start, *caps)
                for con in ((None, None, None), (al[s], fx[s], cp[s])):
                    got = constrained_search_np(*args, start, *con, *caps)
                    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
                    assert list(got[3]) == list(want[3]) + [0, 0] and got[4] == want[4]


def test_feasible_local_optimum_of_both_neighbourhoods():
    """N = 4, M = 3, a random mask, capacities and one fixed UAV: from each of the 4^4 assignments the
    result is feasible, and no feasible single move and no feasible exchange raises J above the
    result's. The bar is rounding only, test_refine_np_reaches_a_local_optimum's: 1e-12 max(1, |J|)."""
    import oracle
    N, M = 4, 3
    allowed, capacity, _ = random_constraints(N, M, 3, seed=6)
    for omega in OMEGAS:
        dropped = conflicts = exchanged = 0
        for e, sc in enumerate(host_scenes(N, M, 3)):
            pd, pp = oracle.score_pairs(sc, prm(omega))
            P = pd * pp[:, None]
            v, c, ids = sc["tgt_value"], sc["uav_cost"], [int(i) for i in sc["tgt_id"]]
            ok, cap = allowed[e].astype(bool), capacity[e]
            fixed = np.zeros(N, np.uint8)
            fixed[e + 1] = 1
            allJ = {a: J_of(P, v, c, omega, a) for a in itertools.product(range(-1, M), repeat=N)}

            def feasible(a, a1):
                """a keeps the fixed UAV of a1, its free pairs are allowed and its targets within
                max(capacity, the fixed UAVs on them)."""
                if any(fixed[u] and a[u] != a1[u] for u in range(N)):
                    return False
                if any(not fixed[u] and a[u] >= 0 and not ok[u][a[u]] for u in range(N)):
                    return False
                return all(sum(x == t for x in a) <= max(cap[t], sum(a[u] == t and fixed[u] for u in range(N)))
                           for t in range(M))

            for a0 in allJ:
                start = np.array([ids[t] if t >= 0 else -1 for t in a0], np.int32)
                out, J, cov, st, _ = constrained_search_np(pd, pp, v, c, sc["tgt_id"], omega, start, ok, fixed, cap)
                a1 = tuple(ids.index(i) if i >= 0 else -1 for i in out)
                tol = RTOL_J * max(1.0, abs(J))
                assert st[2] == 1 and st[3] == 0 and st[5] == 1
                assert abs(J - allJ[a1]) <= tol and cov == len({t for t in a1 if t >= 0})
                check_guarantees((omega, e, a0), out[None], sc["tgt_id"][None], start[None], ok[None], fixed[None],
                                 cap[None])
                assert feasible(a1, a1), (a0, a1)
                for u in range(N):
                    for t in range(-1, M):
                        b = a1[:u] + (t,) + a1[u + 1:]
                        assert not feasible(b, a1) or allJ[b] <= J + tol, (a0, a1, u, t)
                for i, j in itertools.combinations(range(N), 2):
                    sw = list(a1)
                    sw[i], sw[j] = sw[j], sw[i]
                    assert not feasible(tuple(sw), a1) or allJ[tuple(sw)] <= J + tol, (a0, a1, i, j)
                dropped, conflicts, exchanged = dropped + int(st[6]), conflicts + int(st[7]), exchanged + int(st[4] > 0)
        print(f"omega {omega}: {dropped} pairs dropped, {conflicts} fixed conflicts, {exchanged} starts exchanged")
        assert dropped > 0 and conflicts > 0


def test_gpu_case_conditions_on_oracle_tables():
    """The conditions tests/test_gpu_constrained_search.py asserts on its cases (there on the device's
    tables), here on the oracle's, and the guarantees on every output."""
    for (N, M, E), omega in itertools.product(CASE_SHAPES + [EITHER], OMEGAS):
        tabs = oracle_tables(N, M, E, omega)
        allowed, capacity, fixed_ids = random_constraints(N, M, E)
        runs = []
        for base in (None, random_starts(N, M, E)):
            start, fixed = with_fixed(base, fixed_ids)
            runs.append(constrained_rows(*tabs, omega, start, allowed, fixed, capacity, *CAPS))
            check_guarantees((N, M, E, omega), runs[-1][0], tabs[4], start, allowed, fixed, capacity)
        check_constrained_conditions(f"({N}, {M}, {E}) omega {omega}", *runs, tabs[4], capacity,
                                     want=(N, M, E) != EITHER)


def test_binding_signature():
    from uavhip import _lib
    res, args = _lib._SIGS["uavhip_search_assignments_constrained"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), i32, i32, i32, i32] + [vp] * 9
    assert _lib.LIB.uavhip_search_assignments_constrained.argtypes == args
    assert _lib.LIB.uavhip_abi_version() == 6


def test_argument_checks_without_gpu():
    """Every documented misuse of uavhip_search_assignments_constrained returns UAVHIP_EINVAL with a
    message naming the function, before any HIP call (the placeholders would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_search_assignments_constrained, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_search_assignments_constrained"

    def call(env=None, stride=1, S=6, exchanges=4, sweeps=4, allowed=P, fixed=P, cap=P, ain=P, out=P, J=P, cov=P,
             stats=P):
        return fn(env or _env_desc(), stride, S, exchanges, sweeps, allowed, fixed, cap, ain, out, J, cov, stats, None)

    assert call(out=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(J=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(cov=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(stride=0) == -1 and name in err() and b"env_stride=0" in err()
    assert call(stride=-2) == -1 and name in err() and b"env_stride=-2" in err()
    assert call(S=0) == -1 and name in err() and b"S=0" in err()
    assert call(S=7) == -1 and name in err() and b"E=6" in err()              # rows past E
    assert call(stride=3, S=3) == -1 and name in err() and b"E=6" in err()    # (S - 1) * stride = 6 = E
    assert call(stride=1 << 30, S=1 << 30) == -1 and name in err()            # no 32-bit wrap of the product
    assert call(sweeps=-1) == -1 and name in err() and b"max_sweeps=-1" in err()
    assert call(exchanges=-1) == -1 and name in err() and b"max_exchanges=-1" in err()
    assert call(env=_env_desc(N=65)) == -1 and name in err() and b"bad env dims" in err()
    assert call(env=_env_desc(M=129)) == -1 and name in err() and b"bad env dims" in err()
    assert call(allowed=None, fixed=None, cap=None, out=None) == -1 and name in err()  # NULL constraints are no excuse
    assert fn(None, 1, 1, 0, 0, P, P, P, P, P, P, P, P, None) == -1 and name in err()


def test_python_layers_refuse_before_any_device_call():
    import torch

    from uavhip import AllocationSolver, Constraints
    from uavhip.vec_env import VecUAVEnv
    E, N, M = 6, 4, 4
    call = lambda *a, **k: VecUAVEnv.search_assignments_constrained(_HostEnv(E, N, M), *a, **k)  # noqa: E731
    with pytest.raises(ValueError, match="search_assignments_constrained: stride=0"):
        call(stride=0)
    with pytest.raises(ValueError, match="search_assignments_constrained: rows=7"):
        call(rows=7)
    with pytest.raises(ValueError, match="search_assignments_constrained: rows=3 at stride=3"):
        call(stride=3, rows=3)
    with pytest.raises(ValueError, match="max_exchanges=-1"):
        call(max_exchanges=-1)
    with pytest.raises(ValueError, match="max_sweeps=-1"):
        call(max_sweeps=-1)
    with pytest.raises(ValueError, match="assignment: need a contiguous torch.int32"):
        call(torch.zeros(E, N, dtype=torch.int64))
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8"):
        call(allowed=torch.ones(E, N, M, dtype=torch.bool))
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8"):
        call(allowed=torch.ones(E, M, N + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8"):
        call(allowed=torch.ones(E, N, 2 * M, dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8 tensor of 48"):
        call(allowed=torch.ones(E, N, M, dtype=torch.uint8), stride=2)  # row-indexed: 3 rows at stride 2
    with pytest.raises(ValueError, match="fixed: need a contiguous torch.uint8"):
        call(fixed=torch.zeros(E, N, dtype=torch.int32))
    with pytest.raises(ValueError, match="fixed: need a contiguous torch.uint8"):
        call(fixed=torch.zeros(E, N + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="capacity: need a contiguous torch.int32"):
        call(capacity=torch.zeros(E, M, dtype=torch.int64))
    with pytest.raises(ValueError, match="capacity: need a contiguous torch.int32"):
        call(capacity=torch.zeros(E, N + M, dtype=torch.int32))
    with pytest.raises(ValueError, match="stats: need a contiguous torch.int32"):
        call(stats=torch.zeros(E, 6, dtype=torch.int32))  # search_assignments' shape
    with pytest.raises(ValueError, match="J: need a contiguous torch.float64"):
        call(J=torch.zeros(E, dtype=torch.float32))

    class OnGpu(torch.nn.Module):  # stands in for a device policy: only the device is looked at here
        def parameters(self, recurse=True):
            class P:
                device = torch.device("cuda", 0)
            return iter([P()])

    S = 2
    s = AllocationSolver(OnGpu(), N, M, samples=2)
    good = Constraints(allowed=torch.ones(S, N, M, dtype=torch.uint8), capacity=torch.ones(S, M, dtype=torch.int32),
                       fixed_ids=torch.full((S, N), -2, dtype=torch.int32))
    with pytest.raises(ValueError, match="solve: constraints need refine > 0"):
        s.solve(num_scenes=S, refine=0, exchanges=0, constraints=good)
    with pytest.raises(ValueError, match="solve: constraints must be a uavhip.solve.Constraints"):
        s.solve(num_scenes=S, refine=4, constraints={"allowed": None})
    with pytest.raises(ValueError, match="baseline: constraints must be a uavhip.solve.Constraints"):
        s.baseline(num_scenes=S, constraints=(None, None, None))
    bad = {"allowed": (torch.ones(S, N, M, dtype=torch.int32), torch.ones(S, M, N + 1, dtype=torch.uint8)),
           "capacity": (torch.ones(S, M, dtype=torch.int64), torch.ones(S + 1, M, dtype=torch.int32)),
           "fixed_ids": (torch.zeros(S, N, dtype=torch.uint8), np.zeros((S, N + 1), np.int32))}
    for name, values in bad.items():
        for value in values:
            for run in (lambda c: s.solve(num_scenes=S, refine=4, constraints=c),
                        lambda c: s.baseline(num_scenes=S, constraints=c)):
                with pytest.raises(ValueError, match=f"constraints.{name}: need"):
                    run(Constraints(**{name: value}))
    assert s.env is None
