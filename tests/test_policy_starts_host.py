"""Host-side checks of uavhip_search_multistart_from (no GPU): multistart_from_np, the restatement of
the rule (include/uavhip.h) that tests/test_gpu_policy_starts.py compares the kernels against bit for
bit -- R0 given starts per row, each the constrained search from its own start with the fixed UAVs
taken from start 0, then the random replicas of uavhip_search_multistart under their own index r. On
the oracle's tables: R0 = 1 is multistart_np; R0 = R is constrained_search_np per replica; a random
replica does not depend on R0; an id of no target is counted in the replica that was given it. And the
binding, the argument checks of the entry point, of the Python layers above it and of the command line."""
import ctypes
import json

import numpy as np
import pytest

import capi_host
from test_constrained_search_host import check_guarantees, constrained_search_np, random_constraints, with_fixed
from test_exact_host import _OnGpu, convert_ids
from test_multistart_host import _RestartStub, multistart_np, random_start
from test_refine_host import OMEGAS, _env_desc
from test_search_host import _HostEnv, oracle_tables

_entry_point = capi_host._entry_point("uavhip_search_multistart_from")

HOST_SHAPES = [(5, 7, 6), (16, 32, 4)]
GIVEN_SEED = 21


def given_starts(N, M, E, R0, seed=GIVEN_SEED):
    """[E, R0, N] target ids (every id of [0, M) is some target's): start 0 empty; the others random with
    about a quarter -1, and from start 2 on (start 1 when R0 == 2) UAV 0 on an id of no target and UAVs
    1 and 2 on one and the same id."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, M, (E, R0, N)).astype(np.int32)
    a[rng.random((E, R0, N)) < 0.25] = -1
    a[:, 0] = -1
    for r in range(1 if R0 == 2 else 2, R0):
        a[:, r, 0] = M + 3 + r
        a[:, r, 1] = a[:, r, 2] = r % M
    return a


def multistart_from_np(p_dmg, p_pen, value, cost, tgt_id, omega, s, R, R0, seed, starts=None, allowed=None,
                       fixed=None, capacity=None, max_exchanges=32, max_sweeps=32):
    """uavhip_search_multistart_from for row s (one scene), in Python floats. Scene arguments, allowed,
    fixed, capacity as constrained_search_np; starts [R0, N] target ids, or None with R0 == 1.
    -> (replicas: R tuples (assignment [N] int32 target ids, J, covered, stats [8] int32), r*, the number
    of replicas strictly above replica 0's J)."""
    N, M = np.shape(p_dmg)
    assert 1 <= R0 <= R and (starts is not None or R0 == 1)
    first = None if starts is None else np.asarray(starts[0], np.int32)
    fx = np.zeros(N, bool) if fixed is None else np.asarray(fixed).astype(bool)
    con = (allowed, fixed, capacity, max_exchanges, max_sweeps)
    reps = []
    for r in range(R0):
        # the fixed UAVs' ids are start 0's, so the conversion and the count of invalid ids are the
        # constrained search's own on the start the replica is actually given
        start = first if r == 0 else np.where(fx, first, np.asarray(starts[r], np.int32)).astype(np.int32)
        reps.append(constrained_search_np(p_dmg, p_pen, value, cost, tgt_id, omega, start, *con)[:4])
    ids, a0 = convert_ids(tgt_id, first, N)
    for r in range(R0, R):
        rnd = random_start(N, M, r, s, seed)
        a = [a0[u] if fx[u] else rnd[u] for u in range(N)]
        out, J, cov, st, _ = constrained_search_np(p_dmg, p_pen, value, cost, range(M), omega, a, *con)
        st = st.copy()
        st[3] = reps[0][3][3]  # all of start 0 is converted in a random replica
        reps.append((np.array([ids[t] if t >= 0 else -1 for t in out], np.int32), J, cov, st))
    Js = [x[1] for x in reps]
    return reps, Js.index(max(Js)), sum(J > Js[0] for J in Js)


def multistart_from_rows(p_dmg, p_pen, value, cost, tgt_id, omega, R, R0, seed, starts=None, allowed=None, fixed=None,
                         capacity=None, max_exchanges=32, max_sweeps=32):
    """multistart_from_np over rows -> (J_all [S, R], r* [S], above [S], replicas per row)."""
    pick = lambda x, s: None if x is None else x[s]  # noqa: E731
    rows = [multistart_from_np(p_dmg[s], p_pen[s], value[s], cost[s], tgt_id[s], omega, s, R, R0, seed, pick(starts, s),
                               pick(allowed, s), pick(fixed, s), pick(capacity, s), max_exchanges, max_sweeps)
            for s in range(len(p_dmg))]
    return (np.array([[x[1] for x in reps] for reps, _, _ in rows]), np.array([b for _, b, _ in rows]),
            np.array([n for _, _, n in rows]), [reps for reps, _, _ in rows])


def same_replica(x, y):
    return np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2] and list(x[3]) == list(y[3])


def constrained_case(N, M, E, R0):
    """(starts [E, R0, N] with the fixed ids written into start 0 alone, allowed, fixed, capacity)."""
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    starts = given_starts(N, M, E, R0)
    starts[:, 0], fixed = with_fixed(starts[:, 0], fixed_ids)
    return starts, allowed, fixed, capacity


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_one_given_start_is_multistart_np(shape, omega):
    """R0 = 1: multistart_np from starts[0], every replica, the choice and the count; None is the empty start."""
    N, M, E = shape
    tabs = oracle_tables(N, M, E, omega)
    starts, allowed, fixed, capacity = constrained_case(N, M, E, 1)
    for s in range(E):
        args = tuple(t[s] for t in tabs) + (omega, s, 4)
        for given, con in ((None, (None, None, None)), (starts[s], (allowed[s], fixed[s], capacity[s]))):
            got = multistart_from_np(*args, 1, 7, given, *con)
            want = multistart_np(*args, 7, None if given is None else given[0], *con)
            assert got[1:] == want[1:] and all(same_replica(x, y) for x, y in zip(got[0], want[0]))


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_every_given_replica_is_the_constrained_search(shape, omega):
    """R0 = R = 4: replica r is constrained_search_np from start r with start 0's ids on the fixed UAVs;
    the fixed UAVs end where start 0 put them in every replica and the guarantees hold."""
    N, M, E = shape
    tabs = oracle_tables(N, M, E, omega)
    starts, allowed, fixed, capacity = constrained_case(N, M, E, 4)
    for s in range(E):
        args = tuple(t[s] for t in tabs) + (omega,)
        con = (allowed[s], fixed[s], capacity[s])
        reps, best, above = multistart_from_np(*args, s, 4, 4, 7, starts[s], *con)
        ids, a0 = convert_ids(tabs[4][s], starts[s, 0], N)
        for r, rep in enumerate(reps):
            own = np.where(fixed[s] != 0, starts[s, 0], starts[s, r]).astype(np.int32)
            assert same_replica(rep, constrained_search_np(*args, own, *con)[:4]), (shape, omega, s, r)
            check_guarantees((shape, omega, s, r), rep[0][None], tabs[4][s][None], own[None], allowed[s][None],
                             fixed[s][None], capacity[s][None])
            assert all(rep[0][u] == (ids[a0[u]] if a0[u] >= 0 else -1) for u in range(N) if fixed[s, u])
        Js = [x[1] for x in reps]
        assert best == Js.index(max(Js)) and above == sum(J > Js[0] for J in Js)
        free = multistart_from_np(*args, s, 4, 4, 7, starts[s])[0]  # without constraints: each start on its own
        for r, rep in enumerate(free):
            assert same_replica(rep, constrained_search_np(*args, starts[s, r])[:4])


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_random_replicas_do_not_depend_on_r0(shape, omega):
    """Replica r >= R0 is multistart_np's replica r from starts[0], whatever R0 is."""
    N, M, E = shape
    tabs = oracle_tables(N, M, E, omega)
    starts, allowed, fixed, capacity = constrained_case(N, M, E, 3)
    for s in range(min(E, 4)):
        args = tuple(t[s] for t in tabs) + (omega, s, 5)
        con = (allowed[s], fixed[s], capacity[s])
        want = multistart_np(*args, 9, starts[s, 0], *con)[0]
        for R0 in (1, 2, 3):
            got = multistart_from_np(*args, R0, 9, starts[s, :R0], *con)[0]
            assert all(same_replica(got[r], want[r]) for r in [0] + list(range(R0, 5))), (shape, omega, s, R0)


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_invalid_and_duplicated_ids_stay_in_their_replica(shape, omega):
    """given_starts' id of no target in starts 2 and 3 is counted in those replicas alone; with a target
    id that occurs twice in the list, a UAV given it starts on the lower list index and the id the
    duplicate replaced matches nothing."""
    N, M, E = shape
    tabs = oracle_tables(N, M, E, omega)
    starts = given_starts(N, M, E, 4)
    for s in range(E):
        args = tuple(t[s] for t in tabs) + (omega,)
        reps = multistart_from_np(*args, s, 6, 4, 3, starts[s])[0]
        assert [int(x[3][3]) for x in reps] == [0, 0, 1, 1, 0, 0]
        fixed = np.zeros(N, np.uint8)
        fixed[0] = 1  # UAV 0 fixed: its id is start 0's (-1) in every replica, the unknown id is not read
        reps = multistart_from_np(*args, s, 6, 4, 3, starts[s], None, fixed)[0]
        assert [int(x[3][3]) for x in reps] == [0] * 6 and all(x[0][0] == -1 for x in reps)
        twice = tabs[4][s].copy()
        lo, hi = sorted((int(np.flatnonzero(twice == 2)[0]), int(np.flatnonzero(twice == M - 1)[0])))
        gone, twice[hi] = int(twice[hi]), twice[lo]
        own = starts[s].copy()
        own[own == gone] = -1
        own[3, 3], own[3, 4] = twice[lo], gone
        reps = multistart_from_np(*(t[s] for t in tabs[:4]), twice, omega, s, 6, 4, 3, own)[0]
        assert [int(x[3][3]) for x in reps[:2]] == [0, 0] and int(reps[3][3][3]) == 2 and int(reps[5][3][3]) == 0
        alone = constrained_search_np(*(t[s] for t in tabs[:4]), twice, omega, own[3])
        assert same_replica(reps[3], alone[:4])


def test_binding_signature():
    from uavhip import _lib
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    res, args = _lib._SIGS["uavhip_search_multistart_from"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvDesc), i32, i32, i32, i32, u64, i32, i32] + [vp] * 10 + [i64, vp]
    assert _lib.LIB.uavhip_search_multistart_from.argtypes == args
    sibling = _lib._SIGS["uavhip_search_multistart"][1]
    assert args == sibling[:4] + [i32] + sibling[4:]  # the sibling's arguments with R0 after R
    assert _lib.LIB.uavhip_abi_version() == 6 and _lib.MULTISTART_MAX_R == 1024


def test_argument_checks_without_gpu():
    """Every documented misuse of uavhip_search_multistart_from returns UAVHIP_EINVAL with a message
    naming the function and the values, before any HIP call (the placeholders would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_search_multistart_from, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    name = b"uavhip_search_multistart_from"
    enough = int(_lib.LIB.uavhip_multistart_workspace_bytes(6, 4, 8))

    def call(env=None, stride=1, S=6, R=4, R0=2, seed=1, exchanges=4, sweeps=4, allowed=P, fixed=P, cap=P, starts=P,
             out=P, J=P, cov=P, stats=P, J_all=P, ws=P, nbytes=enough):
        return fn(env or _env_desc(), stride, S, R, R0, seed, exchanges, sweeps, allowed, fixed, cap, starts, out, J, cov,
                  stats, J_all, ws, nbytes, None)

    assert call(R0=0) == -1 and name in err() and b"R0=0" in err() and b"R=4" in err()
    assert call(R0=-1) == -1 and name in err() and b"R0=-1" in err()
    assert call(R0=5) == -1 and name in err() and b"R0=5" in err() and b"R=4" in err()
    assert call(R0=2, starts=None) == -1 and name in err() and b"R0=2" in err() and b"starts" in err()
    assert call(R0=4, starts=None) == -1 and name in err() and b"starts" in err()
    # the sibling's cases
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
    assert call(R=0, R0=1) == -1 and name in err() and b"R=0" in err()
    assert call(R=-3, R0=1) == -1 and name in err() and b"R=-3" in err()
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
    assert call(allowed=None, fixed=None, cap=None, stats=None, J_all=None, out=None) == -1 and name in err()
    assert fn(None, 1, 1, 1, 1, 0, 0, 0, P, P, P, P, P, P, P, P, P, P, enough, None) == -1 and name in err()


def test_python_layers_refuse_before_any_device_call():
    import torch

    from uavhip import AllocationSolver
    from uavhip.vec_env import VecUAVEnv
    E, N, M = 6, 4, 4
    call = lambda *a, **k: VecUAVEnv.search_assignments_multistart(_HostEnv(E, N, M), *a, **k)  # noqa: E731
    given = torch.full((E, 3, N), -1, dtype=torch.int32)
    with pytest.raises(ValueError, match="search_assignments_multistart: pass assignment or starts, not both"):
        call(torch.zeros(E, N, dtype=torch.int32), starts=given)
    with pytest.raises(ValueError, match=r"search_assignments_multistart: restarts=2 must be >= the 3 given starts"):
        call(starts=given, restarts=2)
    with pytest.raises(ValueError, match="starts: need a contiguous torch.int32"):
        call(starts=given.long())
    with pytest.raises(ValueError, match="starts: need a contiguous torch.int32"):
        call(starts=torch.full((E, 3, N + 1), -1, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"starts: need a contiguous torch.int32 tensor \[3, R0 >= 1, 4\]"):
        call(starts=given, stride=2)            # row-indexed: 3 rows at stride 2
    with pytest.raises(ValueError, match="starts: need a contiguous torch.int32"):
        call(starts=given[:, 0])                # [rows, N]: that is `assignment`
    with pytest.raises(ValueError, match="starts: need a contiguous torch.int32"):
        call(starts=torch.full((E, 0, N), -1, dtype=torch.int32))
    with pytest.raises(ValueError, match="restarts=0 must be in"):
        call(starts=given, restarts=0)
    with pytest.raises(ValueError, match="search_assignments_multistart: rows=7"):
        call(starts=given, rows=7)

    S = 2
    with pytest.raises(ValueError, match="solve: starts='replicas' needs samples >= 2"):
        AllocationSolver(_OnGpu(), N, M, samples=1).solve(num_scenes=S, refine=4, restarts=4, starts="replicas")
    s = AllocationSolver(_OnGpu(), N, M, samples=4)
    with pytest.raises(ValueError, match="solve: starts='replicas' needs restarts=3 >= samples=4"):
        s.solve(num_scenes=S, refine=4, restarts=3, starts="replicas")
    with pytest.raises(ValueError, match="solve: starts='replicas' needs restarts=0 >= samples=4"):
        s.solve(num_scenes=S, refine=4, starts="replicas")
    with pytest.raises(ValueError, match="solve: restarts > 0 needs refine > 0"):
        s.solve(num_scenes=S, refine=0, restarts=4, starts="replicas")
    for bad in ("all", "", None, 1):
        with pytest.raises(ValueError, match="solve: starts must be 'best' or 'replicas'"):
            s.solve(num_scenes=S, refine=4, restarts=4, starts=bad)
    assert s.env is None


class _StartsStub(_RestartStub):
    """_RestartStub whose solve takes restarts= and starts=: the arguments are recorded."""
    solves = []

    def solve(self, num_scenes, seed, refine=0, exchanges=0, restarts=0, starts="best"):
        import torch
        if starts == "best":
            assert restarts == 0
            return super().solve(num_scenes, seed, refine, exchanges)
        _StartsStub.solves.append((refine, exchanges, restarts, starts))
        r = self._alloc([2.0, 4.0, 3.5, 2.0], [0.5, 1.0, 1.5, 1.0], stats=10)
        r.refine_stats[:, 8] = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
        return r


def test_command_line_starts_keys(monkeypatch, capsys):
    """--starts replicas adds exactly the named keys, its absence (and --starts best) none; what it needs
    is refused before the device is asked for."""
    import torch

    import uavhip.checkpoint
    import uavhip.policy
    from uavhip import solve

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    for bad, msg in ((["--samples", "2"], "--starts replicas needs --restarts R >= --samples K >= 2"),
                     (["--samples", "4", "--restarts", "3"], "--starts replicas needs --restarts R >= --samples K >= 2"),
                     (["--samples", "1", "--restarts", "4"], "--starts replicas needs --restarts R >= --samples K >= 2")):
        with pytest.raises(SystemExit):
            solve.main(["--checkpoint", "x", "--starts", "replicas"] + bad)
        assert msg in capsys.readouterr().err
    with pytest.raises(SystemExit):
        solve.main(["--checkpoint", "x", "--starts", "all"])
    capsys.readouterr()

    class Net:
        def to(self, dev):
            return self
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(uavhip.policy, "TransformerActorCritic", Net)
    monkeypatch.setattr(uavhip.checkpoint, "load_checkpoint", lambda policy, path: None)
    monkeypatch.setattr(solve, "AllocationSolver", _StartsStub)
    argv = ["--checkpoint", "x", "--scenes", "4", "--uavs", "4", "--targets", "4", "--samples", "2", "--restarts", "4"]

    def run(extra):
        solve.main(argv + extra)
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    for extra in ([], ["--optimum"], ["--refine", "4", "--exchanges", "2"], ["--refine", "4", "--optimum"]):
        plain = run(extra)
        assert not [k for k in plain if "policy_start" in k], plain
        best = run(extra + ["--starts", "best"])
        assert list(best) == list(plain) and all(best[k] == plain[k] for k in plain if k != "scenes_per_s")
        _StartsStub.solves.clear()
        out = run(extra + ["--starts", "replicas"])
        new = [k for k in out if k not in plain]
        want = ["mean_J_policy_starts", "policy_start_wins", "policy_starts_beat_random"]
        if "--optimum" in extra:
            want += ["policy_starts_over_optimal", "policy_starts_is_optimal"]
        assert new == want, (extra, new)
        assert [k for k in out if k in plain] == list(plain)  # the existing keys keep their order
        assert all(out[k] == plain[k] for k in plain if k != "scenes_per_s")
        # the stub: J 2, 4, 3.5, 2 from replicas 0, 1, 2, 3 of K = 2 given; the multi-start baseline 2, 4, 3, 1
        assert out["mean_J_policy_starts"] == 2.875 and out["policy_start_wins"] == 0.5
        assert out["policy_starts_beat_random"] == 0.5
        assert _StartsStub.solves == [(4 if "--refine" in extra else 32, 2 if "--exchanges" in extra else 32, 4, "replicas")]
        if "--optimum" in extra:
            assert out["policy_starts_over_optimal"] == 2.875 / 2.75 and out["policy_starts_is_optimal"] == 1.0
