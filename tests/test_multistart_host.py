"""Host-side checks of uavhip_search_multistart (no GPU): multistart_np, the restatement of the rule
(include/uavhip.h) that tests/test_gpu_multistart.py compares the kernels against bit for bit -- a
Python Philox4x32-10 checked against the published known answers, the start rule, constrained_search_np
(tests/test_constrained_search_host.py) per replica and the choice of the replica; R = 1 is the
constrained search exactly; the two counts a CPU run of this rule gave on the oracle's tables; never
above the exact optimum; fixed UAVs and the constraints in every replica; and the argument checks of
the entry points, of the Python layers above them and of the command line."""
import ctypes
import functools
import json

import numpy as np
import pytest

import capi_host
from test_constrained_search_host import check_guarantees, constrained_search_np, random_constraints, with_fixed
from test_exact_host import _OnGpu, _StubSolver, convert_ids, exact_np
from test_refine_host import OMEGAS, RTOL_J, _env_desc, random_starts
from test_search_host import CAPS, _HostEnv, oracle_tables, search_np

_entry_point = capi_host._entry_point("uavhip_search_multistart")

STREAM = 0x5354524D  # the fourth counter word of the start rule ("STRM")
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123): counter [4], key [2] of uint32 -> [4] uint32."""
    c0, c1, c2, c3 = (int(x) & M32 for x in counter)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def random_start(N, M, r, s, seed):
    """The list indices replica r >= 1 of row s starts its free UAVs on."""
    key = (seed & M32, (seed >> 32) & M32)
    return [(philox4x32_10((u >> 2, r, s, STREAM), key)[u & 3] * M) >> 32 for u in range(N)]


def multistart_np(p_dmg, p_pen, value, cost, tgt_id, omega, s, R, seed, start=None, allowed=None, fixed=None,
                  capacity=None, max_exchanges=32, max_sweeps=32):
    """uavhip_search_multistart for row s (one scene), in Python floats. Scene arguments, start, allowed,
    fixed, capacity as constrained_search_np.
    -> (replicas: R tuples (assignment [N] int32 target ids, J, covered, stats [8] int32), r*, the number
    of replicas strictly above replica 0's J)."""
    N, M = np.shape(p_dmg)
    reps = [constrained_search_np(p_dmg, p_pen, value, cost, tgt_id, omega, start, allowed, fixed, capacity,
                                  max_exchanges, max_sweeps)[:4]]
    ids, a0 = convert_ids(tgt_id, start, N)
    fx = [False] * N if fixed is None else [bool(x) for x in fixed]
    for r in range(1, R):
        rnd = random_start(N, M, r, s, seed)
        a = [a0[u] if fx[u] else rnd[u] for u in range(N)]
        # a list-index start: the same rule on ids 0..M-1, where the conversion is the identity
        out, J, cov, st, _ = constrained_search_np(p_dmg, p_pen, value, cost, range(M), omega, a, allowed, fixed,
                                                   capacity, max_exchanges, max_sweeps)
        st = st.copy()
        st[3] = reps[0][3][3]  # the invalid ids of the input, converted in every replica
        reps.append((np.array([ids[t] if t >= 0 else -1 for t in out], np.int32), J, cov, st))
    Js = [x[1] for x in reps]
    return reps, Js.index(max(Js)), sum(J > Js[0] for J in Js)


def multistart_rows(p_dmg, p_pen, value, cost, tgt_id, omega, R, seed, starts=None, allowed=None, fixed=None,
                    capacity=None, max_exchanges=32, max_sweeps=32):
    """multistart_np over rows -> (J_all [S, R], r* [S], above [S], replicas per row)."""
    pick = lambda x, s: None if x is None else x[s]  # noqa: E731
    rows = [multistart_np(p_dmg[s], p_pen[s], value[s], cost[s], tgt_id[s], omega, s, R, seed, pick(starts, s),
                          pick(allowed, s), pick(fixed, s), pick(capacity, s), max_exchanges, max_sweeps)
            for s in range(len(p_dmg))]
    return (np.array([[x[1] for x in reps] for reps, _, _ in rows]), np.array([b for _, b, _ in rows]),
            np.array([n for _, _, n in rows]), [reps for reps, _, _ in rows])


def test_philox_known_answers():
    """The known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10)."""
    hexs = lambda x: " ".join(f"{w:08x}" for w in x)  # noqa: E731
    assert hexs(philox4x32_10([0] * 4, [0] * 2)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexs(philox4x32_10([M32] * 4, [M32] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexs(philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_random_starts_are_list_indices():
    """0 <= t < M for every UAV, M = 1 and 128 included; the key's two halves and r, s all matter."""
    for N, M in ((1, 1), (5, 7), (64, 128), (33, 34)):
        a = random_start(N, M, 3, 2, 5)
        assert len(a) == N and all(0 <= t < M for t in a)
    base = random_start(64, 128, 1, 0, 0)
    assert len(set(base)) > 32
    for other in (random_start(64, 128, 2, 0, 0), random_start(64, 128, 1, 1, 0), random_start(64, 128, 1, 0, 1),
                  random_start(64, 128, 1, 0, 1 << 32)):
        assert other != base


def test_one_replica_is_the_constrained_search():
    """R = 1: constrained_search_np exactly, and without constraints search_np."""
    N, M, E = 5, 7, 6
    for omega in OMEGAS:
        tabs = oracle_tables(N, M, 33, omega)
        starts = random_starts(N, M, 33)
        allowed, capacity, fixed_ids = random_constraints(N, M, 33)
        start, fixed = with_fixed(starts, fixed_ids)
        for s in range(E):
            args = tuple(t[s] for t in tabs) + (omega,)
            reps, best, above = multistart_np(*args, s, 1, 9, starts[s])
            want = search_np(*args, starts[s], *CAPS)
            assert best == 0 and above == 0 and len(reps) == 1
            assert np.array_equal(reps[0][0], want[0]) and reps[0][1] == want[1] and reps[0][2] == want[2]
            assert list(reps[0][3]) == list(want[3]) + [0, 0]
            reps, best, above = multistart_np(*args, s, 1, 9, start[s], allowed[s], fixed[s], capacity[s])
            want = constrained_search_np(*args, start[s], allowed[s], fixed[s], capacity[s], *CAPS)
            assert best == 0 and above == 0
            assert np.array_equal(reps[0][0], want[0]) and reps[0][1:3] == want[1:3] and list(reps[0][3]) == list(want[3])


@functools.lru_cache(maxsize=None)
def headline_rows(omega):
    """oracle_tables(16, 32, 32, omega), seed 0, R = 16, caps 32 / 32: multistart_rows' result."""
    return multistart_rows(*oracle_tables(16, 32, 32, omega), omega, 16, 0)


@pytest.mark.parametrize("omega,rows_above,mean0,mean16", [(0.0, 13, 26.73355, 26.78219), (0.5, 11, 19.98942, 20.04158)])
def test_cpu_checked_counts(omega, rows_above, mean0, mean16):
    """16 x 32 x 32, seed 0, R = 16: never below replica 0; strictly above it in at least 8 rows (a CPU
    run of this rule: 13 rows at omega = 0, 11 at 0.5, mean J 26.73355 -> 26.78219 and 19.98942 ->
    20.04158)."""
    J_all, best, above, _ = headline_rows(omega)
    J = J_all[np.arange(len(best)), best]
    better = int((J > J_all[:, 0]).sum())
    print(f"omega {omega}: {better} rows above replica 0, mean J {J_all[:, 0].mean():.5f} -> {J.mean():.5f}, "
          f"replicas above per row {above.tolist()}")
    assert bool((J >= J_all[:, 0]).all()) and bool((J == J_all.max(1)).all())
    assert better >= 8
    assert bool(((above > 0) == (J > J_all[:, 0])).all())
    assert better == rows_above and abs(J_all[:, 0].mean() - mean0) < 1e-5 and abs(J.mean() - mean16) < 1e-5


@pytest.mark.parametrize("N,M,E", [(4, 4, 6), (10, 12, 3)])
def test_never_above_the_exact_optimum(N, M, E):
    """N <= 10: no replica's J exceeds exact_np's optimum beyond RTOL_J, unconstrained and constrained."""
    for omega in OMEGAS:
        tabs = oracle_tables(N, M, E, omega)
        allowed, capacity, fixed_ids = random_constraints(N, M, E)
        start, fixed = with_fixed(None, fixed_ids)
        for con in ((None, None, None, None), (start, allowed, fixed, capacity)):
            J_all = multistart_rows(*tabs, omega, 5, 3, *con)[0]
            for s in range(E):
                _, Jx = exact_np(*(t[s] for t in tabs), omega, *(None if x is None else x[s] for x in con))
                assert J_all[s].max() <= Jx + RTOL_J * max(1.0, abs(Jx)), (N, M, omega, s, J_all[s], Jx)


@pytest.mark.parametrize("N,M,E", [(5, 7, 33), (16, 32, 4)])
def test_fixed_uavs_and_constraints_in_every_replica(N, M, E):
    """random_constraints' cases: in every replica a fixed UAV leaves with the id it came with, no
    forbidden or over-capacity pair survives, and some random start had a pair dropped."""
    tabs = oracle_tables(N, M, E, 0.5)
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    start, fixed = with_fixed(random_starts(N, M, E), fixed_ids)
    rows = range(min(E, 6))
    dropped = 0
    for s in rows:
        reps, best, _ = multistart_np(*(t[s] for t in tabs), 0.5, s, 5, 1, start[s], allowed[s], fixed[s], capacity[s])
        for r, (asg, J, cov, st) in enumerate(reps):
            check_guarantees((N, M, s, r), asg[None], tabs[4][s][None], start[s][None], allowed[s][None],
                             fixed[s][None], capacity[s][None])
            dropped += int(st[6]) if r else 0
            assert st[7] == reps[0][3][7] and st[3] == reps[0][3][3]  # pass 1 sees the same fixed UAVs
    assert dropped > 0


def test_binding_signature():
    from uavhip import _lib
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    res, args = _lib._SIGS["uavhip_search_multistart"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), i32, i32, i32, u64, i32, i32] + [vp] * 10 + [i64, vp]
    assert _lib.LIB.uavhip_search_multistart.argtypes == args
    assert _lib._SIGS["uavhip_multistart_workspace_bytes"] == (i64, [i32, i32, i32])
    assert _lib.LIB.uavhip_multistart_workspace_bytes.restype is i64
    assert _lib.LIB.uavhip_abi_version() == 6 and _lib.MULTISTART_MAX_R == 1024


def test_workspace_bytes():
    from uavhip import _lib
    need = _lib.LIB.uavhip_multistart_workspace_bytes
    # per replica: J (8), covered (4), N ids (4 N), eight counters (32); the total rounded up to 16
    assert need(4096, 16, 16) == 4096 * 16 * (44 + 4 * 16)
    assert need(1, 1, 1) == 48 and need(3, 5, 64) == 3 * 5 * (44 + 256) + 12 and need(1, 1024, 64) == 1024 * 300
    assert need(1 << 20, 1024, 4) == (1 << 30) * 60
    for bad in ((0, 4, 4), (4, 0, 4), (4, 1025, 4), (4, 4, 0), (4, 4, 65), (-1, 4, 4), (4, -2, 4), ((1 << 20) + 1, 1024, 4)):
        assert need(*bad) == -1, bad


def test_argument_checks_without_gpu():
    """Every documented misuse of uavhip_search_multistart returns UAVHIP_EINVAL with a message naming
    the function, before any HIP call (the placeholders would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_search_multistart, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_search_multistart"
    enough = int(_lib.LIB.uavhip_multistart_workspace_bytes(6, 4, 8))

    def call(env=None, stride=1, S=6, R=4, seed=1, exchanges=4, sweeps=4, allowed=P, fixed=P, cap=P, ain=P, out=P, J=P,
             cov=P, stats=P, J_all=P, ws=P, nbytes=enough):
        return fn(env or _env_desc(), stride, S, R, seed, exchanges, sweeps, allowed, fixed, cap, ain, out, J, cov, stats,
                  J_all, ws, nbytes, None)

    assert call(out=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(J=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(cov=None) == -1 and name in err() and b"non-NULL" in err()
    assert call(stride=0) == -1 and name in err() and b"env_stride=0" in err()
    assert call(stride=-2) == -1 and name in err() and b"env_stride=-2" in err()
    assert call(S=0) == -1 and name in err() and b"S=0" in err()
    assert call(S=7, nbytes=1 << 30) == -1 and name in err() and b"E=6" in err()   # rows past E
    assert call(stride=3, S=3) == -1 and name in err() and b"E=6" in err()         # (S - 1) * stride = 6 = E
    assert call(stride=1 << 30, S=1 << 30) == -1 and name in err()                 # no 32-bit wrap of the product
    assert call(sweeps=-1) == -1 and name in err() and b"max_sweeps=-1" in err()
    assert call(exchanges=-1) == -1 and name in err() and b"max_exchanges=-1" in err()
    assert call(R=0) == -1 and name in err() and b"R=0" in err()
    assert call(R=-3) == -1 and name in err() and b"R=-3" in err()
    assert call(R=1025, nbytes=1 << 40) == -1 and name in err() and b"R=1025" in err()
    assert call(env=_env_desc(N=65)) == -1 and name in err() and b"bad env dims" in err()
    assert call(env=_env_desc(M=129)) == -1 and name in err() and b"bad env dims" in err()
    assert call(nbytes=enough - 1) == -1 and name in err() and b"workspace" in err()   # one byte short
    assert call(R=5) == -1 and name in err() and b"workspace" in err()                  # sized for 4 replicas
    assert call(nbytes=0) == -1 and name in err() and b"workspace" in err()
    assert call(nbytes=-5) == -1 and name in err() and b"workspace" in err()
    assert call(ws=None) == -1 and name in err() and b"workspace" in err()
    assert call(ws=ctypes.c_void_p(24)) == -1 and name in err() and b"aligned" in err()
    assert call(env=_env_desc(E=1 << 21), S=(1 << 20) + 1, R=1024, nbytes=1 << 50) == -1 and b"2^30" in err()
    assert call(allowed=None, fixed=None, cap=None, ain=None, stats=None, J_all=None, out=None) == -1 and name in err()
    assert fn(None, 1, 1, 1, 0, 0, 0, P, P, P, P, P, P, P, P, P, P, enough, None) == -1 and name in err()


def test_python_layers_refuse_before_any_device_call():
    import torch

    from uavhip import AllocationSolver
    from uavhip.vec_env import VecUAVEnv
    E, N, M = 6, 4, 4
    call = lambda *a, **k: VecUAVEnv.search_assignments_multistart(_HostEnv(E, N, M), *a, **k)  # noqa: E731
    with pytest.raises(ValueError, match="search_assignments_multistart: stride=0"):
        call(stride=0)
    with pytest.raises(ValueError, match="search_assignments_multistart: rows=7"):
        call(rows=7)
    with pytest.raises(ValueError, match="search_assignments_multistart: rows=3 at stride=3"):
        call(stride=3, rows=3)
    with pytest.raises(ValueError, match="max_exchanges=-1"):
        call(max_exchanges=-1)
    with pytest.raises(ValueError, match="max_sweeps=-1"):
        call(max_sweeps=-1)
    for R in (0, -1, 1025):
        with pytest.raises(ValueError, match=f"restarts={R} must be in"):
            call(restarts=R)
    with pytest.raises(ValueError, match="seed=-1 must be in"):
        call(seed=-1)
    with pytest.raises(ValueError, match="assignment: need a contiguous torch.int32"):
        call(torch.zeros(E, N, dtype=torch.int64))
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8"):
        call(allowed=torch.ones(E, N, M, dtype=torch.bool))
    with pytest.raises(ValueError, match="allowed: need a contiguous torch.uint8 tensor of 48"):
        call(allowed=torch.ones(E, N, M, dtype=torch.uint8), stride=2)  # row-indexed: 3 rows at stride 2
    with pytest.raises(ValueError, match="fixed: need a contiguous torch.uint8"):
        call(fixed=torch.zeros(E, N + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="capacity: need a contiguous torch.int32"):
        call(capacity=torch.zeros(E, M, dtype=torch.int64))
    with pytest.raises(ValueError, match="J_all: need a contiguous torch.float64"):
        call(J_all=torch.zeros(E, 16, dtype=torch.float32))
    with pytest.raises(ValueError, match="J_all: need a contiguous torch.float64"):
        call(J_all=torch.zeros(E, 16, dtype=torch.float64), restarts=4)
    with pytest.raises(ValueError, match="stats: need a contiguous torch.int32"):
        call(stats=torch.zeros(E, 8, dtype=torch.int32))  # the constrained search's shape
    with pytest.raises(ValueError, match="J: need a contiguous torch.float64"):
        call(J=torch.zeros(E, dtype=torch.float32))

    S = 2
    s = AllocationSolver(_OnGpu(), N, M, samples=2)
    with pytest.raises(ValueError, match="solve: restarts > 0 needs refine > 0"):
        s.solve(num_scenes=S, restarts=4)
    with pytest.raises(ValueError, match="solve: restarts must be in"):
        s.solve(num_scenes=S, refine=4, restarts=-1)
    with pytest.raises(ValueError, match="solve: restarts must be in"):
        s.solve(num_scenes=S, refine=4, restarts=1025)
    with pytest.raises(ValueError, match="baseline: restarts must be in"):
        s.baseline(num_scenes=S, restarts=-1)
    with pytest.raises(ValueError, match="baseline: constraints must be a uavhip.solve.Constraints"):
        s.baseline(num_scenes=S, restarts=4, constraints=(None, None, None))
    assert s.env is None


class _RestartStub(_StubSolver):
    """_StubSolver with baseline(restarts=): the arguments are recorded."""
    seen = []

    def baseline(self, num_scenes, seed, exchanges=0, restarts=0):
        if restarts:
            _RestartStub.seen.append((exchanges, restarts))
            return self._alloc([2.0, 4.0, 3.0, 1.0], stats=10)
        return super().baseline(num_scenes, seed, exchanges)


def test_command_line_restarts_keys(monkeypatch, capsys):
    """--restarts adds exactly the named keys (and --baseline's), its absence none; the cap is
    --exchanges' or 32; a value out of range is refused before the device is asked for."""
    import torch

    import uavhip.checkpoint
    import uavhip.policy
    from uavhip import solve

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    for bad in ("-1", "1025"):
        with pytest.raises(SystemExit):
            solve.main(["--checkpoint", "x", "--restarts", bad])
        assert "--restarts must be in" in capsys.readouterr().err

    class Net:
        def to(self, dev):
            return self
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(uavhip.policy, "TransformerActorCritic", Net)
    monkeypatch.setattr(uavhip.checkpoint, "load_checkpoint", lambda policy, path: None)
    monkeypatch.setattr(solve, "AllocationSolver", _RestartStub)
    argv = ["--checkpoint", "x", "--scenes", "4", "--uavs", "4", "--targets", "4"]

    def run(extra):
        solve.main(argv + extra)
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    for extra in ([], ["--baseline"], ["--optimum"], ["--refine", "4", "--baseline", "--exchanges", "2", "--optimum"]):
        plain = run(extra)
        assert not [k for k in plain if "multistart" in k], plain
        _RestartStub.seen.clear()
        with_r = run(extra + ["--restarts", "4"])
        new = [k for k in with_r if k not in plain]
        want = ["mean_J_multistart"]
        if "--baseline" not in extra and "--optimum" not in extra:
            want = ["mean_J_baseline", "policy_beats_baseline"] + want  # --restarts implies --baseline
        if "--optimum" in extra:
            want += ["multistart_over_optimal", "multistart_is_optimal"]
        assert new == want, (extra, new)
        assert [k for k in with_r if k in plain] == list(plain)  # the existing keys keep their order
        assert all(with_r[k] == plain[k] for k in plain if k != "scenes_per_s")
        assert with_r["mean_J_multistart"] == 2.5
        assert _RestartStub.seen == [(2 if "--exchanges" in extra else 32, 4)]
        if "--optimum" in extra:
            assert with_r["multistart_over_optimal"] == 2.5 / 2.75 and with_r["multistart_is_optimal"] == 0.75
