"""Host-side checks of uavhip_refine_assignments (no GPU): refine_np, the numpy restatement of the
best-response rule (include/uavhip.h) that tests/test_gpu_refine.py compares the kernel against bit
for bit; its local optimality on scenes small enough to enumerate; its J against the oracle env's;
the cases the GPU tests run; and the entry point's argument checks."""
import ctypes
import functools
import itertools
import random

import numpy as np
import pytest

import capi_host
from capi_host import _env_desc

RTOL_J = 1e-12  # the project's reward bar
SHAPES = [(4, 4, 6), (5, 7, 33), (16, 32, 32), (33, 34, 3), (3, 70, 5)]  # (N, M, E); the last: two targets per lane
OMEGAS = (0.0, 0.5)
SCENE_SEED, START_SEED = 7, 1


_entry_point = capi_host._entry_point("uavhip_refine_assignments")


def refine_np(p_dmg, p_pen, value, cost, tgt_id, omega, start=None, max_sweeps=32):
    """uavhip_refine_assignments for one scene, in Python floats (IEEE doubles, one rounding per
    operation, nothing contracted). p_dmg [N, M], p_pen [N], value [M], cost [N], tgt_id [M];
    start [N] target ids or -1 (None: all -1).
    -> (assignment [N] int32 target ids, J, covered, stats [4] int32 = sweeps, moves, converged,
    invalid ids, moves in sweeps >= 2, moves to -1)."""
    N, M = np.shape(p_dmg)
    P = [[float(p_dmg[u][t]) * float(p_pen[u]) for t in range(M)] for u in range(N)]
    v, c, omega = [float(x) for x in value], [float(x) for x in cost], float(omega)
    ids = [int(x) for x in tgt_id]
    a, invalid = [-1] * N, 0
    if start is not None:
        for u in range(N):
            want = int(start[u])
            if want == -1:
                continue
            if want in ids:
                a[u] = ids.index(want)  # the lowest list index of a duplicated id
            else:
                invalid += 1

    def products(skip):
        """Q[t] over the UAVs w != skip on t, ascending w, from 1.0; and their number."""
        Q, cnt = [1.0] * M, [0] * M
        for w in range(N):
            if w != skip and a[w] >= 0:
                Q[a[w]] = Q[a[w]] * (1.0 - P[w][a[w]])
                cnt[a[w]] += 1
        return Q, cnt

    sweeps = moves = late = to_none = 0
    converged = 1
    while sweeps < max_sweeps:
        moved = False
        for u in range(N):
            Q, _ = products(u)
            g = [(v[t] * Q[t]) * P[u][t] - (omega * c[u]) for t in range(M)]
            cur = g[a[u]] if a[u] >= 0 else 0.0
            cand, gain = -1, 0.0
            for t in range(M):
                if g[t] > gain:
                    cand, gain = t, g[t]
            if gain > cur:
                a[u] = cand
                moved = True
                moves += 1
                late += sweeps >= 1
                to_none += cand < 0
        sweeps += 1
        converged = int(not moved)
        if not moved:
            break
    Q, cnt = products(-1)
    J = 0.0
    for t in range(M):
        if cnt[t]:
            J = J + v[t] * (1.0 - Q[t])
    csum = 0.0
    for u in range(N):
        if a[u] >= 0:
            csum = csum + c[u]
    J = J - omega * csum
    out = np.array([ids[t] if t >= 0 else -1 for t in a], np.int32)
    return out, J, sum(1 for n in cnt if n), np.array([sweeps, moves, converged, invalid], np.int32), late, to_none


def prm(omega):
    from uavhip import _lib
    from uavhip.config import cfg, params_vector
    p = np.array(params_vector(cfg), np.float64)
    p[_lib.PRM["OMEGA"]] = omega
    return p


@functools.lru_cache(maxsize=None)
def host_scenes(N, M, n, seed=SCENE_SEED):
    from uavhip.config import Config
    from uavhip.scene import generate_scene
    c = Config()
    c.NUM_UAVS, c.NUM_TARGETS = N, M
    np.random.seed(seed)
    random.seed(seed)
    return tuple(generate_scene(c) for _ in range(n))


def random_starts(N, M, E, seed=START_SEED):
    """[E, N] target ids in [0, M) with about a quarter -1 (every id of [0, M) is some target's)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, M, (E, N)).astype(np.int32)
    a[rng.random((E, N)) < 0.25] = -1
    return a


def refine_rows(p_dmg, p_pen, value, cost, tgt_id, omega, starts, max_sweeps=32):
    """refine_np over rows: (assignment [S, N], J [S], covered [S], stats [S, 4], late [S], to_none [S])."""
    rows = [refine_np(p_dmg[s], p_pen[s], value[s], cost[s], tgt_id[s], omega, None if starts is None else starts[s],
                      max_sweeps) for s in range(len(p_dmg))]
    return tuple(np.array([r[i] for r in rows]) for i in range(6))


def check_case_conditions(label, runs):
    """The conditions of a GPU case (one shape at one omega; runs = refine_rows results of its
    starts): some scene moves a UAV in sweep >= 2, at omega > 0 some move goes to -1 (the caller
    says so), every run converges within its 32 sweeps."""
    late = sum(int((r[4] > 0).sum()) for r in runs)
    to_none = sum(int(r[5].sum()) for r in runs)
    total = sum(len(r[1]) for r in runs)
    sweeps = max(int(r[3][:, 0].max()) for r in runs)
    print(f"{label}: {late} of {total} runs move in sweep >= 2, {to_none} moves to -1, at most {sweeps} sweeps")
    assert late > 0, label
    assert all(bool((r[3][:, 2] == 1).all()) for r in runs), label
    return to_none


def J_of(P, v, c, omega, a):
    J = 0.0
    for t in range(len(v)):
        Q, n = 1.0, 0
        for u in range(len(c)):
            if a[u] == t:
                Q, n = Q * (1.0 - P[u][t]), n + 1
        if n:
            J += v[t] * (1.0 - Q)
    return J - omega * sum(c[u] for u in range(len(c)) if a[u] >= 0)


def test_refine_np_reaches_a_local_optimum():
    """N = 4, M = 3: from each of the 4^4 assignments the result is never below the start's J, and no
    single-UAV move raises J above the result's. The bar is rounding only: J is a sum of at most
    M + 1 terms of magnitude <= 16 (the largest target value), so 1e-12 max(1, |J|) is > 1000 ulp."""
    import oracle
    N, M = 4, 3
    for omega in OMEGAS:
        worst_gap = 0.0
        for sc in host_scenes(N, M, 3):
            pd, pp = oracle.score_pairs(sc, prm(omega))
            P = pd * pp[:, None]
            v, c, ids = sc["tgt_value"], sc["uav_cost"], [int(i) for i in sc["tgt_id"]]
            allJ = {a: J_of(P, v, c, omega, a) for a in itertools.product(range(-1, M), repeat=N)}
            best = max(allJ.values())
            for a0, J0 in allJ.items():
                start = [ids[t] if t >= 0 else -1 for t in a0]
                out, J, cov, st, _, _ = refine_np(pd, pp, v, c, sc["tgt_id"], omega, start)
                a1 = tuple(ids.index(i) if i >= 0 else -1 for i in out)
                tol = RTOL_J * max(1.0, abs(J))
                assert st[2] == 1 and st[3] == 0
                assert abs(J - allJ[a1]) <= tol and cov == len({t for t in a1 if t >= 0})
                assert J >= J0 - tol, (a0, J0, J)
                for u in range(N):
                    for t in range(-1, M):
                        assert allJ[a1[:u] + (t,) + a1[u + 1:]] <= J + tol, (a0, a1, u, t)
                worst_gap = max(worst_gap, best - J)
        print(f"omega {omega}: largest gap of a local optimum to the global optimum {worst_gap:.4f}")


def test_refine_np_scores_like_the_env():
    """max_sweeps = 0 on an allocation the oracle env built: J is the env's J (_calc_J_X) to the reward
    bar, covered its num_assigned, and nothing moves."""
    import oracle
    rng = np.random.default_rng(3)
    for (N, M), omega in itertools.product([(4, 4), (5, 7), (16, 32)], OMEGAS):
        for sc in host_scenes(N, M, 2):
            ref = oracle.OracleEnv(sc, prm(omega))
            ref.reset()
            done = False
            while not done:
                _, _, done, info = ref.step(int(rng.random() < 0.5))
            pd, pp = oracle.score_pairs(sc, prm(omega))
            ids = ref.assigned()
            out, J, cov, st, _, _ = refine_np(pd, pp, sc["tgt_value"], sc["uav_cost"], sc["tgt_id"], omega, ids, 0)
            assert (ids >= 0).any() and np.array_equal(out, ids) and list(st) == [0, 0, 1, 0]
            assert abs(J - info[0]) <= RTOL_J * max(1.0, abs(info[0])), (J, info[0])
            assert cov == int(info[1])


def test_refine_np_counts_invalid_ids_and_caps_sweeps():
    import oracle
    N, M = 5, 7
    sc = host_scenes(N, M, 1)[0]
    pd, pp = oracle.score_pairs(sc, prm(0.5))
    args = (pd, pp, sc["tgt_value"], sc["uav_cost"], sc["tgt_id"], 0.5)
    out, J, cov, st, _, _ = refine_np(*args, [0, 99, -1, -7, 3], 0)
    assert list(out) == [0, -1, -1, -1, 3] and st[3] == 2
    full = refine_np(*args, None, 32)
    one = refine_np(*args, None, 1)
    # from the empty assignment the first sweep moves, so a cap of one sweep cannot see convergence
    assert full[3][0] >= 2 and full[3][2] == 1 and list(one[3][[0, 2]]) == [1, 0] and one[3][1] > 0


def test_gpu_case_conditions_on_oracle_tables():
    """The conditions tests/test_gpu_refine.py asserts on its cases (there on the device's tables),
    here on the oracle's, for the empty and the random starts."""
    import oracle
    for (N, M, E), omega in itertools.product(SHAPES, OMEGAS):
        scenes = host_scenes(N, M, E)
        tabs = [oracle.score_pairs(sc, prm(omega)) for sc in scenes]
        pd, pp = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
        v, c, ids = (np.stack([sc[k] for sc in scenes]) for k in ("tgt_value", "uav_cost", "tgt_id"))
        runs = [refine_rows(pd, pp, v, c, ids, omega, st) for st in (None, random_starts(N, M, E))]
        to_none = check_case_conditions(f"({N}, {M}, {E}) omega {omega}", runs)
        assert omega == 0.0 or to_none > 0


def test_refine_argument_checks_without_gpu():
    """Every documented misuse of uavhip_refine_assignments returns UAVHIP_EINVAL with a message naming
    the function, before any HIP call (the placeholders would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_refine_assignments, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_refine_assignments"

    def call(env=None, stride=1, S=6, sweeps=4, ain=P, out=P, J=P, cov=P, stats=P):
        return fn(env or _env_desc(), stride, S, sweeps, ain, out, J, cov, stats, None)

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
    assert call(env=_env_desc(N=65)) == -1 and name in err() and b"bad env dims" in err()
    assert call(env=_env_desc(M=129)) == -1 and name in err() and b"bad env dims" in err()
    assert fn(None, 1, 1, 0, P, P, P, P, P, None) == -1 and name in err()


def test_refine_binding_and_solver_arguments():
    """The Python layers refuse what they can see without a device."""
    import dataclasses

    import torch

    from uavhip import AllocationSolver
    from uavhip.solve import Allocation

    class OnGpu(torch.nn.Module):  # stands in for a device policy: only the device is looked at here
        def parameters(self, recurse=True):
            class P:
                device = torch.device("cuda", 0)
            return iter([P()])

    s = AllocationSolver(OnGpu(), 4, 4, samples=2)
    with pytest.raises(ValueError, match="refine"):
        s.solve(num_scenes=2, refine=-1)
    with pytest.raises(ValueError, match="baseline: pass scenes or num_scenes"):
        s.baseline()
    names = [f.name for f in dataclasses.fields(Allocation)]
    assert names[-2:] == ["decoded_J", "refine_stats"]
    z = torch.zeros(2)
    a = Allocation(z, z, z, z, z, z).cpu()
    assert a.decoded_J is None and a.refine_stats is None and a.actions is None
    b = Allocation(z, z, z, z, z, z, decoded_J=z + 1, refine_stats=z + 2).cpu()
    assert float(b.decoded_J[0]) == 1 and float(b.refine_stats[0]) == 2
