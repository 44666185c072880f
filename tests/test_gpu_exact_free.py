"""uavhip_solve_exact_free and uavhip_neighbourhood_pick on the GPU (k_exact_free_* / k_neighbourhood_pick):
the kernels' J against exact_free_np and the picks against pick_np byte for byte (tests/test_exact_free_host.py),
fed the pair tables read back from the device; with every UAV free, every output bitwise uavhip_solve_exact's;
and on the kernels' own outputs J bitwise the scoring call's, the guarantees of the constrained search, the
held UAVs where they came from, stats, overflow, chunks and two launches bitwise equal. Above them
VecUAVEnv.lns_assignments (never below its start, reproducible, the host loop's J, a captured graph) and
AllocationSolver's lns_rounds.

Shapes (N, M, E, max_free, share of UAVs held at random): 5 x 7 with 33 rows, the smallest tables and a
partial last workgroup; 16 x 32, the workload's shape; 20 x 6 with 11 bits, N > 16 and one high bit (two
tiles a row); 33 x 34, lanes beyond 32; 3 x 70, two targets per lane; 64 x 128, the full range; 24 x 2 with
16 bits, every bit of a choice entry and 3^16 steps a target."""
import functools

import numpy as np
import pytest
import torch

import capi_host
from test_constrained_search_host import check_guarantees, random_constraints
from test_exact_free_host import (RANDOM, TARGETS, exact_free_rows, free_list, held_case, lns_np, pick_np)
from test_exact_host import constraint_cases, convert_ids
from test_gpu_refine import make_env, tables
from test_gpu_solve import gpu_policy
from test_refine_host import OMEGAS, RTOL_J, host_scenes, random_starts

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 33, 3, 0.4), (16, 32, 8, 6, 0.4), (20, 6, 3, 11, 0.3), (33, 34, 3, 8, 0.4), (3, 70, 5, 3, 0.2),
          (64, 128, 2, 4, 0.4), (24, 2, 1, 16, 0.1)]
N_CASES = 7        # test_exact_host.constraint_cases
NEVER_WORSE_SEED = 4  # chosen on the CPU with exact_free_np: row 0 of 16 x 32 ends above the exchange search

_entry_point = capi_host._entry_point("uavhip_solve_exact_free")


def dev(env, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(env.device)


def bar(J):
    return RTOL_J * np.maximum(1.0, np.abs(J))


@functools.lru_cache(maxsize=None)
def scene_env(N, M, E, omega):
    """(the env of host_scenes(N, M, E) at omega, its tables as numpy): shared, never written."""
    env = make_env(host_scenes(N, M, E), N, M, omega)
    return env, tables(env)


def launch(env, max_free, start=None, allowed=None, fixed=None, capacity=None, **kw):
    got = env.exact_free_assignments(dev(env, start), max_free=max_free, allowed=dev(env, allowed), fixed=dev(env, fixed),
                                     capacity=dev(env, capacity), **kw)
    torch.cuda.synchronize()
    return got


def check_own_outputs(label, env, tabs, got, max_free, start, allowed, fixed, capacity):
    """What the header promises of the outputs themselves: J, covered and the ids bitwise the scoring
    call's; the guarantees with every held UAV (fixed or overflow) a fixed one."""
    asg, J, cov, st = got
    scored = env.refine_assignments(asg, max_sweeps=0)
    torch.cuda.synchronize()
    assert asg.dtype == torch.int32 and torch.equal(scored[0], asg), label
    assert torch.equal(scored[1], J) and torch.equal(scored[2], cov), label        # bitwise
    N = asg.shape[1]
    held = np.stack([free_list(N, None if fixed is None else fixed[s], max_free)[1] for s in range(len(J))]).astype(np.uint8)
    check_guarantees(label, asg.cpu().numpy(), tabs[4], start, allowed, held, capacity)
    return held


def run_and_compare(label, env, tabs, omega, max_free, start, allowed, fixed, capacity):
    """One launch against exact_free_np on the device's tables: J to the reward bar, stats exactly."""
    got = launch(env, max_free, start, allowed, fixed, capacity)
    _, want, want_stats = exact_free_rows(*tabs, omega, max_free, start, allowed, fixed, capacity)
    J = got[1].cpu().numpy()
    err = np.abs(J - want) / np.maximum(1.0, np.abs(want))
    print(f"{label}: {len(J)} rows, mean J {want.mean():.6f}, max J err {err.max():.2e} (bar {RTOL_J:g}), "
          f"stats sum {want_stats.sum(0).tolist()}")
    assert bool((err <= RTOL_J).all()), (label, float(err.max()))
    assert got[3].shape == (len(J), 4) and np.array_equal(got[3].cpu().numpy(), want_stats), label
    check_own_outputs(label, env, tabs, got, max_free, start, allowed, fixed, capacity)
    return got, want, want_stats


@pytest.mark.parametrize("allowed_and_capacity", (False, True))
@pytest.mark.parametrize("N,M,E", [(5, 7, 3), (12, 6, 3), (16, 4, 2)])
def test_all_free_is_solve_exact_bitwise(N, M, E, allowed_and_capacity):
    """N <= 16, fixed = None, max_free = N (and above): every output, stats columns 0-1 included, is
    uavhip_solve_exact's bit for bit, from the empty start and from ids with an invalid one."""
    for omega in OMEGAS:
        env, _ = scene_env(N, M, E, omega)
        allowed, capacity, _ = random_constraints(N, M, E) if allowed_and_capacity else (None, None, None)
        start = random_starts(N, M, E)
        start[0, 0] = M + 3
        for st in (None, start):
            want = env.exact_assignments(dev(env, st), dev(env, allowed), None, dev(env, capacity))
            for max_free in {N, 16}:
                got = launch(env, max_free, st, allowed, None, capacity)
                for x, y in zip(got[:3], want[:3]):
                    assert torch.equal(x, y), (N, M, omega, max_free)
                assert torch.equal(got[3][:, :2], want[3]) and bool((got[3][:, 2] == N).all()) and not bool(got[3][:, 3].any())


@pytest.mark.parametrize("case", range(N_CASES))
@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_reaches_the_numpy_optimum(shape, omega, case):
    """Every constraint case of test_exact_host.constraint_cases merged with a random held set; J against
    the restatement, stats, the guarantees, the held UAVs as they came. Assignments are compared through J
    only: the DP's rounding order is the kernel's own."""
    N, M, E, max_free, p_held = shape
    env, tabs = scene_env(N, M, E, omega)
    cs = constraint_cases(N, M, E)[case]
    start, allowed, fixed, capacity = held_case(cs, N, M, E, p_held)
    label = f"({N}, {M}, {E}) K = {max_free} omega {omega} {cs[0]}"
    got, _, stats = run_and_compare(label, env, tabs, omega, max_free, start, allowed, fixed, capacity)
    if case == 0:
        assert stats[:, 2].max() == min(max_free, N), label   # some row fills every bit of the table
    ids, asg = tabs[4], got[0].cpu().numpy()
    for s in range(E):   # a held UAV leaves with the id it came with (an id of no target as -1)
        for u in np.flatnonzero(fixed[s]):
            came = int(start[s][u])
            assert int(asg[s][u]) == (came if came in ids[s].tolist() else -1), (label, s, u)


@pytest.mark.parametrize("omega", OMEGAS)
def test_overflow_is_held(omega):
    """More free UAVs than max_free: the extra ones are held where they came from, stats column 3 counts
    them, and the result is that of the call with them fixed."""
    N, M, E, max_free = 16, 32, 8, 6
    env, tabs = scene_env(N, M, E, omega)
    start = random_starts(N, M, E)
    fixed = np.zeros((E, N), np.uint8)
    fixed[:, 1] = fixed[:, 4] = 1
    got, _, stats = run_and_compare(f"overflow omega {omega}", env, tabs, omega, max_free, start, None, fixed, None)
    assert bool((stats[:, 2] == max_free).all()) and bool((stats[:, 3] == N - 2 - max_free).all())
    explicit = np.stack([free_list(N, fixed[s], max_free)[1] for s in range(E)]).astype(np.uint8)
    same = launch(env, max_free, start, None, explicit, None)
    for x, y in zip(got[:3], same[:3]):
        assert torch.equal(x, y)
    assert not bool(same[3][:, 3].any())
    assert torch.equal(got[0][:, 8:], dev(env, start)[:, 8:])  # UAVs 0, 2, 3, 5, 6, 7 are the DP's; 8.. are held
    none = launch(env, max_free)                               # the empty start: every held UAV on none
    assert bool((none[0][:, 6:] == -1).all()) and bool((none[3][:, 3] == N - max_free).all())


def test_chunks_and_repeat():
    """A workspace of one row gives the outputs of a workspace of all rows, bitwise; so does a second call;
    caller buffers are used; the env and the inputs are only read."""
    N, M, E, max_free, omega = 20, 6, 3, 11, 0.5
    env, _ = scene_env(N, M, E, omega)
    from uavhip import _lib
    row = int(_lib.LIB.uavhip_exact_free_workspace_bytes(max_free, M, 1))
    start, allowed, fixed, capacity = held_case(constraint_cases(N, M, E)[1], N, M, E, 0.3)
    names = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")
    before = {k: getattr(env, k).clone() for k in names}
    before.update({"scene/" + k: t.clone() for k, t in env._scene.items()})
    whole = launch(env, max_free, start, allowed, fixed, capacity)
    for nbytes in (row, 2 * row + 5, None):
        part = launch(env, max_free, start, allowed, fixed, capacity, max_workspace_bytes=nbytes)
        for x, y in zip(whole, part):
            assert torch.equal(x, y), nbytes
    con = [dev(env, x) for x in (start, allowed, fixed, capacity)]
    kept = [x.clone() for x in con]
    bufs = dict(out=torch.empty(E, N, dtype=torch.int32, device=env.device),
                J=torch.empty(E, dtype=torch.float64, device=env.device),
                covered=torch.empty(E, dtype=torch.int32, device=env.device),
                stats=torch.empty(E, 4, dtype=torch.int32, device=env.device))
    mine = env.exact_free_assignments(con[0], max_free=max_free, allowed=con[1], fixed=con[2], capacity=con[3], **bufs)
    torch.cuda.synchronize()
    for x, y, z in zip(mine, whole, bufs.values()):
        assert x.data_ptr() == z.data_ptr() and torch.equal(x, y)
    for x, y in zip(con, kept):
        assert torch.equal(x, y)
    for k in names:
        assert torch.equal(getattr(env, k), before[k]), k
    for k, t in env._scene.items():
        assert torch.equal(t, before["scene/" + k]), k


@pytest.mark.parametrize("omega", OMEGAS)
def test_never_below_the_exchange_search(omega):
    """From the exchange search's result with a random max_free-set of each row free: J >= the input's J to
    the reward bar in every row, and row 0 ends strictly above it (by 0.095 at omega = 0 and 0.158 at 0.5
    on the CPU, exact_free_np on the oracle's tables): the reference alone shows both."""
    N, M, E, max_free = 16, 32, 8, 6
    env, tabs = scene_env(N, M, E, omega)
    found = env.search_assignments(None)
    torch.cuda.synchronize()
    rng = np.random.default_rng(NEVER_WORSE_SEED)
    fixed = np.ones((E, N), np.uint8)
    for s in range(E):
        fixed[s, rng.permutation(N)[:max_free]] = 0
    start = found[0].cpu().numpy()
    got, want, _ = run_and_compare(f"from the search omega {omega}", env, tabs, omega, max_free, start, None, fixed, None)
    J0, J = found[1].cpu().numpy(), got[1].cpu().numpy()
    print(f"omega {omega}: search {J0.tolist()}, neighbourhood optimum {J.tolist()}")
    for x in (want, J):
        assert bool((x >= J0 - bar(J0)).all())
        assert x[0] > J0[0] + 1e-3 and int((x > J0 + bar(J0)).sum()) >= 1


@pytest.mark.parametrize("N,M,E", [(5, 7, 33), (16, 32, 8), (33, 34, 3), (3, 70, 5), (64, 128, 2)])
def test_pick_is_the_restatement(N, M, E):
    """fixed_out byte for byte pick_np's: both modes, three rounds, two seeds (one with a high half),
    K below and above the open UAVs, with and without fixed_in, ids with -1 and an id of no target."""
    env, tabs = scene_env(N, M, E, 0.5)
    start = random_starts(N, M, E)
    start[0, 0] = M + 3
    a = [convert_ids(tabs[4][s], start[s], N)[1] for s in range(E)]
    fixed_in = (np.random.default_rng(2).random((E, N)) < 0.3).astype(np.uint8)
    for mode, name in ((RANDOM, "random"), (TARGETS, "targets")):
        for K, fx, round, seed in ((1, None, 0, 0), (6, fixed_in, 1, 7), (16, None, 2, 7 + (5 << 32)), (12, fixed_in, 2, 7)):
            got = env.pick_neighbourhood(dev(env, start), K, name, round, seed, fixed=dev(env, fx))
            torch.cuda.synchronize()
            want = np.stack([pick_np(N, M, K, mode, round, seed, s, a[s], None if fx is None else fx[s]) for s in range(E)])
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (N, M, name, K, round, seed)
    # no assignment: every UAV idle; fixed_out may be fixed_in itself
    got = env.pick_neighbourhood(None, 3, "targets", 0, 1)
    want = np.stack([pick_np(N, M, 3, TARGETS, 0, 1, s) for s in range(E)])
    assert np.array_equal(got.cpu().numpy(), want)
    buf = dev(env, fixed_in)
    env.pick_neighbourhood(dev(env, start), 6, "targets", 1, 7, fixed=buf, out=buf)
    want = np.stack([pick_np(N, M, 6, TARGETS, 1, 7, s, a[s], fixed_in[s]) for s in range(E)])
    assert np.array_equal(buf.cpu().numpy(), want)


@pytest.mark.parametrize("mode", ("random", "targets"))
def test_lns_against_the_host_loop(mode):
    """12 x 24, 4 rows, K = 6, 4 rounds from the exchange search under constraints and from the empty
    start: never below the start in any row, in the doubles themselves; equal seeds give equal results;
    J is the host loop's (pick_np + exact_free_np, kept where strictly greater) to the reward bar; and a
    captured graph replays the eager call."""
    N, M, E, K, rounds, omega, seed = 12, 24, 4, 6, 4, 0.5, 3
    env, tabs = scene_env(N, M, E, omega)
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    fixed = (fixed_ids != -2).astype(np.uint8)
    base = np.where(fixed_ids != -2, fixed_ids, -1).astype(np.int32)
    found = env.search_assignments_constrained(dev(env, base), dev(env, allowed), dev(env, fixed), dev(env, capacity))
    empty = torch.full((E, N), -1, dtype=torch.int32, device=env.device)
    for start, con in ((found[0], (allowed, fixed, capacity)), (empty, (None, None, None))):
        kw = dict(rounds=rounds, free=K, mode=mode, seed=seed, allowed=dev(env, con[0]), fixed=dev(env, con[1]),
                  capacity=dev(env, con[2]))
        J0 = env.refine_assignments(start, max_sweeps=0)[1]
        kept = start.clone()
        got = env.lns_assignments(start, **kw)
        torch.cuda.synchronize()
        assert torch.equal(start, kept) and bool((got[1] >= J0).all())          # exactly
        assert got[3].dtype == torch.int32 and bool(((got[3] > 0) == (got[1] > J0)).all()) and int(got[3].max()) <= rounds
        scored = env.refine_assignments(got[0], max_sweeps=0)
        assert torch.equal(scored[1], got[1]) and torch.equal(scored[2], got[2]) and torch.equal(scored[0], got[0])
        check_guarantees(mode, got[0].cpu().numpy(), tabs[4], start.cpu().numpy(), con[0], con[1], con[2])
        for x, y in zip(got, env.lns_assignments(start, **kw)):
            assert torch.equal(x, y)
        other = env.lns_assignments(start, **dict(kw, seed=seed + 1))
        host = np.array([lns_np(*(t[s] for t in tabs), omega, s, start[s].cpu().numpy(), rounds, K,
                                TARGETS if mode == "targets" else RANDOM, seed,
                                *(None if x is None else x[s] for x in con))[1] for s in range(E)])
        J = got[1].cpu().numpy()
        print(f"{mode}: start {J0.tolist()}, lns {J.tolist()}, host {host.tolist()}, other seed {other[1].tolist()}")
        assert bool((np.abs(J - host) <= bar(host)).all()), (mode, J, host)
        if con[0] is None:
            assert bool((got[1] > J0).all())   # from the empty start every row improves
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):   # warm-up outside capture (allocator)
                env.lns_assignments(start, **kw)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                replayed = env.lns_assignments(start, **kw)
            g.replay()
            torch.cuda.synchronize()
            for x, y in zip(got, replayed):
                assert torch.equal(x, y)


def test_through_the_solver():
    """lns_rounds = 0 is the call without the argument, bitwise; lns_rounds > 0 is lns_assignments on the
    call's own result under the same constraints, with the J going in kept in lns_J_before."""
    from uavhip import AllocationSolver, Constraints
    N, M, S, K = 16, 32, 4, 2
    solver = AllocationSolver(gpu_policy(N, M, 1), N, M, samples=K)
    fields = lambda r: (r.assignment, r.J, r.covered, r.best_replica, r.steps, r.replica_J, r.decoded_J,  # noqa: E731
                        r.refine_stats)
    for kw in (dict(), dict(refine=8, exchanges=4)):
        plain = solver.solve(num_scenes=S, seed=5, **kw)
        same = solver.solve(num_scenes=S, seed=5, lns_rounds=0, lns_free=3, lns_mode="random", **kw)
        assert plain.lns_J_before is None and same.lns_J_before is None
        for x, y in zip(fields(plain), fields(same)):
            assert (x is None and y is None) or torch.equal(x, y)
        up = solver.solve(num_scenes=S, seed=5, lns_rounds=3, lns_free=8, **kw)
        assert torch.equal(up.lns_J_before, plain.J) and bool((up.J >= plain.J).all())
        direct = solver.env.lns_assignments(plain.assignment, rounds=3, free=8, mode="targets", seed=5, stride=K, rows=S)
        for x, y in zip((up.assignment, up.J, up.covered), direct[:3]):
            assert torch.equal(x, y)
        for x, y in zip(fields(up)[3:], fields(plain)[3:]):
            assert (x is None and y is None) or torch.equal(x, y)
    allowed, capacity, fixed_ids = random_constraints(N, M, S)
    con = Constraints(allowed=torch.from_numpy(allowed), capacity=capacity, fixed_ids=torch.from_numpy(fixed_ids))
    for c in (None, con):
        base = solver.baseline(num_scenes=S, seed=5, exchanges=32, constraints=c)
        same = solver.baseline(num_scenes=S, seed=5, exchanges=32, constraints=c, lns_rounds=0)
        for x, y in zip(fields(base), fields(same)):
            assert (x is None and y is None) or torch.equal(x, y)
        up = solver.baseline(num_scenes=S, seed=5, exchanges=32, constraints=c, lns_rounds=4, lns_free=8, lns_mode="random")
        assert torch.equal(up.lns_J_before, base.J) and bool((up.J >= base.J).all())
        fixed = None if c is None else (fixed_ids != -2).astype(np.uint8)
        check_guarantees("baseline + lns", up.assignment.cpu().numpy(), tables(solver.env, K, S)[4],
                         None if c is None else np.where(fixed_ids != -2, fixed_ids, -1), None if c is None else allowed,
                         fixed, None if c is None else capacity)
        opt = solver.optimum(num_scenes=S, seed=5, constraints=c)
        assert bool((up.J <= opt.J + RTOL_J * opt.J.abs().clamp(min=1.0)).all())
        print(f"constraints {c is not None}: baseline {base.J.tolist()}, + lns {up.J.tolist()}, optimum {opt.J.tolist()}")
