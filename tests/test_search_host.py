"""Host-side checks of uavhip_search_assignments (no GPU): search_np, the restatement of the
exchange-move rule (include/uavhip.h) in Python floats that tests/test_gpu_search.py compares the kernel
against bit for bit -- its best-response phases are refine_np's (tests/test_refine_host.py), imported;
its local optimality in both neighbourhoods on scenes small enough to enumerate; the cases the GPU
tests run; and the argument checks of the entry point and of the Python layers above it."""
import ctypes
import itertools

import numpy as np
import pytest

import capi_host
from test_refine_host import (OMEGAS, RTOL_J, J_of, _env_desc, host_scenes, prm, random_starts, refine_np)

# (N, M, E): every one has a row that makes an exchange; the last two have two targets per lane
SHAPES = [(5, 7, 33), (16, 32, 32), (33, 34, 3), (12, 70, 5), (34, 66, 2)]
NOTHING_TO_DO = (4, 4, 6)  # no row makes an exchange
CAPS = (32, 32)            # max_exchanges, max_sweeps


_entry_point = capi_host._entry_point("uavhip_search_assignments")


def best_exchange(P, v, wc, a):
    """The scan of the rule: (d, i, j) of the pair i < j with a[i] != a[j] and the largest d, the
    lowest i then the lowest j among equal d; None without such a pair."""
    N = len(a)
    Qo = []
    for u in range(N):
        q = 1.0
        if a[u] >= 0:
            for k in range(N):
                if k != u and a[k] == a[u]:
                    q = q * (1.0 - P[k][a[u]])
        Qo.append(q)

    def g(u, x, Q):
        return 0.0 if x < 0 else (v[x] * Q) * P[u][x] - wc[u]

    best = None
    for i in range(N):
        for j in range(i + 1, N):
            s, t = a[i], a[j]
            if s == t:
                continue
            d = (g(j, s, Qo[i]) + g(i, t, Qo[j])) - (g(i, s, Qo[i]) + g(j, t, Qo[j]))
            if best is None or d > best[0]:
                best = (d, i, j)
    return best


def search_np(p_dmg, p_pen, value, cost, tgt_id, omega, start=None, max_exchanges=32, max_sweeps=32):
    """uavhip_search_assignments for one scene, in Python floats. Arguments as refine_np.
    -> (assignment [N] int32 target ids, J, covered, stats [6] int32 = sweeps, moves, phase_converged,
    invalid ids, exchanges, scan_clean; J after every phase (list))."""
    N, M = np.shape(p_dmg)
    P = [[float(p_dmg[u][t]) * float(p_pen[u]) for t in range(M)] for u in range(N)]
    v, omega = [float(x) for x in value], float(omega)
    wc = [omega * float(x) for x in cost]
    ids = [int(x) for x in tgt_id]
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
    sweeps = moves = x = 0
    trace = []
    while True:
        # a phase is refine_np on list indices (ids 0..M-1: the conversion is the identity)
        out, J, cov, st, _, _ = refine_np(p_dmg, p_pen, value, cost, range(M), omega, a, max_sweeps)
        a = [int(t) for t in out]
        sweeps, moves, converged = sweeps + int(st[0]), moves + int(st[1]), int(st[2])
        assert st[3] == 0
        trace.append(J)
        if max_exchanges == 0:
            clean = 0
            break
        best = best_exchange(P, v, wc, a)
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
    return out, J, cov, np.array([sweeps, moves, converged, invalid, x, clean], np.int32), trace


def search_rows(p_dmg, p_pen, value, cost, tgt_id, omega, starts, max_exchanges=32, max_sweeps=32):
    """search_np over rows: (assignment [S, N], J [S], covered [S], stats [S, 6], traces (list of lists))."""
    rows = [search_np(p_dmg[s], p_pen[s], value[s], cost[s], tgt_id[s], omega, None if starts is None else starts[s],
                      max_exchanges, max_sweeps) for s in range(len(p_dmg))]
    return tuple(np.array([r[i] for r in rows]) for i in range(4)) + ([r[4] for r in rows],)


def check_search_conditions(label, runs, want_exchange=True, want_two=False):
    """The conditions of a case (one shape at one omega; runs = search_rows results of its starts) at
    caps 32 / 32: every row ends with phase_converged == scan_clean == 1, J never drops from phase
    to phase beyond the reward bar, some row makes an exchange (want_exchange; False: none does; None: either),
    and some row makes at least two (want_two)."""
    ex = np.concatenate([r[3][:, 4] for r in runs])
    print(f"{label}: {int((ex > 0).sum())} of {len(ex)} rows exchange, at most {int(ex.max())} exchanges, "
          f"mean J {np.concatenate([r[1] for r in runs]).mean():.6f}")
    for r in runs:
        assert bool((r[3][:, 2] == 1).all()) and bool((r[3][:, 5] == 1).all()), label
        assert bool((r[3][:, 4] < CAPS[0]).all()), label
        for tr in r[4]:
            for J0, J1 in zip(tr, tr[1:]):
                assert J1 >= J0 - RTOL_J * max(1.0, abs(J0)), (label, tr)
    assert want_exchange is None or bool((ex > 0).any()) == want_exchange, label
    assert not want_two or int(ex.max()) >= 2, label


def oracle_tables(N, M, E, omega):
    import oracle
    scenes = host_scenes(N, M, E)
    tabs = [oracle.score_pairs(sc, prm(omega)) for sc in scenes]
    pd, pp = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
    return (pd, pp) + tuple(np.stack([sc[k] for sc in scenes]) for k in ("tgt_value", "uav_cost", "tgt_id"))


def test_search_np_reaches_a_local_optimum_of_both_neighbourhoods():
    """N = 4, M = 3: from each of the 4^4 assignments the result is never below the start's J, and
    neither a single-UAV move nor a pairwise exchange raises J above the result's. The bar is rounding
    only, test_refine_np_reaches_a_local_optimum's: 1e-12 max(1, |J|)."""
    import oracle
    N, M = 4, 3
    for omega in OMEGAS:
        exchanged = 0
        for sc in host_scenes(N, M, 3):
            pd, pp = oracle.score_pairs(sc, prm(omega))
            P = pd * pp[:, None]
            v, c, ids = sc["tgt_value"], sc["uav_cost"], [int(i) for i in sc["tgt_id"]]
            allJ = {a: J_of(P, v, c, omega, a) for a in itertools.product(range(-1, M), repeat=N)}
            for a0, J0 in allJ.items():
                start = [ids[t] if t >= 0 else -1 for t in a0]
                out, J, cov, st, _ = search_np(pd, pp, v, c, sc["tgt_id"], omega, start)
                a1 = tuple(ids.index(i) if i >= 0 else -1 for i in out)
                tol = RTOL_J * max(1.0, abs(J))
                assert st[2] == 1 and st[3] == 0 and st[5] == 1
                assert abs(J - allJ[a1]) <= tol and cov == len({t for t in a1 if t >= 0})
                assert J >= J0 - tol, (a0, J0, J)
                for u in range(N):
                    for t in range(-1, M):
                        assert allJ[a1[:u] + (t,) + a1[u + 1:]] <= J + tol, (a0, a1, u, t)
                for i, j in itertools.combinations(range(N), 2):
                    sw = list(a1)
                    sw[i], sw[j] = sw[j], sw[i]
                    assert allJ[tuple(sw)] <= J + tol, (a0, a1, i, j)
                exchanged += int(st[4] > 0)
        print(f"omega {omega}: {exchanged} of {3 * 4 ** N} starts made an exchange")


def test_search_np_without_exchanges_is_refine_np():
    import oracle
    for (N, M, E), omega in itertools.product([(5, 7, 6), (16, 32, 4), (3, 70, 2)], OMEGAS):
        starts = random_starts(N, M, E)
        starts[0, 0] = M + 3  # an id of no target
        for e, sc in enumerate(host_scenes(N, M, E)):
            pd, pp = oracle.score_pairs(sc, prm(omega))
            args = (pd, pp, sc["tgt_value"], sc["uav_cost"], sc["tgt_id"], omega)
            for start, sweeps in ((None, 32), (starts[e], 32), (starts[e], 1), (starts[e], 0)):
                want = refine_np(*args, start, sweeps)
                got = search_np(*args, start, 0, sweeps)
                assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
                assert list(got[3]) == list(want[3]) + [0, 0] and got[4] == [want[1]]


def test_gpu_case_conditions_on_oracle_tables():
    """The conditions tests/test_gpu_search.py asserts on its cases (there on the device's tables),
    here on the oracle's, for the empty and the random starts."""
    for (N, M, E), omega in itertools.product(SHAPES, OMEGAS):
        tabs = oracle_tables(N, M, E, omega)
        runs = [search_rows(*tabs, omega, st, *CAPS) for st in (None, random_starts(N, M, E))]
        check_search_conditions(f"({N}, {M}, {E}) omega {omega}", runs, want_two=(N, M) == (16, 32))
    N, M, E = NOTHING_TO_DO
    for omega in OMEGAS:
        tabs = oracle_tables(N, M, E, omega)
        runs = [search_rows(*tabs, omega, st, *CAPS) for st in (None, random_starts(N, M, E))]
        check_search_conditions(f"({N}, {M}, {E}) omega {omega}", runs, want_exchange=False)


def test_binding_signature():
    from uavhip import _lib
    res, args = _lib._SIGS["uavhip_search_assignments"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), i32, i32, i32, i32] + [vp] * 6
    assert _lib.LIB.uavhip_search_assignments.argtypes == args
    assert _lib.LIB.uavhip_abi_version() == 6


def test_search_argument_checks_without_gpu():
    """Every documented misuse of uavhip_search_assignments returns UAVHIP_EINVAL with a message naming
    the function, before any HIP call (the placeholders would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_search_assignments, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_search_assignments"

    def call(env=None, stride=1, S=6, exchanges=4, sweeps=4, ain=P, out=P, J=P, cov=P, stats=P):
        return fn(env or _env_desc(), stride, S, exchanges, sweeps, ain, out, J, cov, stats, None)

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
    assert fn(None, 1, 1, 0, 0, P, P, P, P, P, None) == -1 and name in err()


class _HostEnv:
    """VecUAVEnv.search_assignments' checks run before any device call: a stand-in with the attributes they read."""

    def __init__(self, E, N, M):
        import torch
        self.E, self.N, self.M, self.device = E, N, M, torch.device("cpu")


def test_python_layers_refuse_before_any_device_call(tmp_path, monkeypatch):
    import torch

    from uavhip import AllocationSolver, imitate
    from uavhip.vec_env import VecUAVEnv
    E, N, M = 6, 4, 4
    call = lambda *a, **k: VecUAVEnv.search_assignments(_HostEnv(E, N, M), *a, **k)  # noqa: E731
    with pytest.raises(ValueError, match="search_assignments: stride=0"):
        call(stride=0)
    with pytest.raises(ValueError, match="search_assignments: rows=7"):
        call(rows=7)
    with pytest.raises(ValueError, match="search_assignments: rows=3 at stride=3"):
        call(stride=3, rows=3)
    with pytest.raises(ValueError, match="max_exchanges=-1"):
        call(max_exchanges=-1)
    with pytest.raises(ValueError, match="max_sweeps=-1"):
        call(max_sweeps=-1)
    with pytest.raises(ValueError, match="assignment: need a contiguous torch.int32"):
        call(torch.zeros(E, N, dtype=torch.int64))
    with pytest.raises(ValueError, match="assignment: need a contiguous torch.int32"):
        call(torch.zeros(E, N + 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="stats: need a contiguous torch.int32"):
        call(stats=torch.zeros(E, 4, dtype=torch.int32))  # refine_assignments' shape
    with pytest.raises(ValueError, match="J: need a contiguous torch.float64"):
        call(J=torch.zeros(E, dtype=torch.float32))

    class OnGpu(torch.nn.Module):  # stands in for a device policy: only the device is looked at here
        def parameters(self, recurse=True):
            class P:
                device = torch.device("cuda", 0)
            return iter([P()])

    s = AllocationSolver(OnGpu(), 4, 4, samples=2)
    with pytest.raises(ValueError, match="solve: exchanges must be >= 0"):
        s.solve(num_scenes=2, refine=4, exchanges=-1)
    with pytest.raises(ValueError, match="exchanges > 0 needs refine > 0"):
        s.solve(num_scenes=2, refine=0, exchanges=4)
    with pytest.raises(ValueError, match="baseline: exchanges must be >= 0"):
        s.baseline(num_scenes=2, exchanges=-1)
    assert s.env is None

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    out = str(tmp_path / "o")
    args = dict(envs=64, uavs=4, targets=4, minibatch=64, out_dir=out)
    with pytest.raises(ValueError, match="teacher_exchanges=-1"):
        imitate.ImitationRun(**args, teacher_exchanges=-1)
    for source in ("expert", "dagger"):
        with pytest.raises(ValueError, match="teacher_exchanges=4: source='teacher' only"):
            imitate.ImitationRun(**args, source=source, teacher_exchanges=4)
    assert not (tmp_path / "o").exists()
    # the arguments pass, and only then is the device asked for
    with pytest.raises(AssertionError, match="a device was touched"):
        imitate.ImitationRun(**args, teacher_exchanges=4)
    with pytest.raises(SystemExit):
        imitate.main(["--iterations", "1", "--out", out, "--teacher-exchanges", "x"])
