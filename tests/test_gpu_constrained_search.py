"""uavhip_search_assignments_constrained on the GPU (k_search_constrained): the kernel against
constrained_search_np, the Python restatement of the constrained rule
(tests/test_constrained_search_host.py), fed the pair tables read back from the device -- assignments,
all eight stats and covered exactly, J to the project's reward bar -- with the guarantees of the header
asserted on the kernel's own outputs; bitwise k_search / k_refine without constraints; and the layers
above it: VecUAVEnv.search_assignments_constrained and AllocationSolver.solve / baseline(constraints=).

Shapes (N, M, E): the register-column path at its three capacities (5 x 7: 8; 16 x 32: 16; 17 x 20: 32),
the streamed path (33 x 34) and two targets per lane (12 x 70, 34 x 66, 8 x 128) -- all five
instantiations; every E but 32 leaves the last workgroup of four waves partial."""
import numpy as np
import pytest
import torch

import capi_host
from test_constrained_search_host import (CASE_SHAPES, check_constrained_conditions, check_guarantees,
                                          constrained_rows, neutral_constraints, random_constraints, with_fixed)
from test_gpu_refine import decoded_env, make_env, tables
from test_gpu_solve import gpu_policy
from test_refine_host import OMEGAS, RTOL_J, host_scenes, random_starts
from test_search_host import CAPS

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 33), (16, 32, 32), (17, 20, 5), (33, 34, 3), (12, 70, 5), (34, 66, 2), (8, 128, 3)]


_entry_point = capi_host._entry_point("uavhip_search_assignments_constrained")


def dev(env, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(env.device)


def run_and_compare(label, env, omega, start, allowed, fixed, capacity, stride=1, rows=None, max_exchanges=CAPS[0],
                    max_sweeps=CAPS[1], **kw):
    """One launch against constrained_search_np on the device's tables, and the guarantees on what the
    launch wrote. Returns (the restatement's rows, the launch's outputs)."""
    got = env.search_assignments_constrained(dev(env, start), dev(env, allowed), dev(env, fixed), dev(env, capacity),
                                             stride=stride, rows=rows, max_exchanges=max_exchanges,
                                             max_sweeps=max_sweeps, **kw)
    torch.cuda.synchronize()
    asg, J, cov, st = (t.cpu().numpy() for t in got)
    tabs = tables(env, stride, rows)
    want = constrained_rows(*tabs, omega, start, allowed, fixed, capacity, max_exchanges, max_sweeps)
    err = np.abs(J - want[1]) / np.maximum(1.0, np.abs(want[1]))
    print(f"{label}: {len(J)} rows, sweeps {want[3][:, 0].min()}..{want[3][:, 0].max()}, exchanges "
          f"{want[3][:, 4].min()}..{want[3][:, 4].max()}, dropped {int(want[3][:, 6].sum())}, fixed conflicts "
          f"{int(want[3][:, 7].sum())}, mean J {want[1].mean():.6f}, max J err {err.max():.2e} (bar {RTOL_J:g})")
    assert asg.dtype == np.int32 and np.array_equal(asg, want[0]), label
    assert st.shape == (len(J), 8) and np.array_equal(st, want[3]), label
    assert np.array_equal(cov, want[2]), label
    assert bool((err <= RTOL_J).all()), (label, float(err.max()))
    check_guarantees(label, asg, tabs[4], start, allowed, fixed, capacity)
    return want, got


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_is_the_restatement(shape, omega):
    """Seeded constraints (mask density 0.7, capacities in {1, 2, 3}, a fifth of the UAVs committed), from
    the empty start and from random ids; and each constraint alone, the other arrays NULL."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    tag = f"({N}, {M}, {E}) omega {omega}"
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    runs = []
    for name, base in (("empty", None), ("random ids", random_starts(N, M, E))):
        start, fixed = with_fixed(base, fixed_ids)
        want, _ = run_and_compare(f"{tag} from {name}", env, omega, start, allowed, fixed, capacity)
        runs.append(want)
    check_constrained_conditions(tag, *runs, tables(env)[4], capacity, want=shape in CASE_SHAPES)
    run_and_compare(f"{tag} allowed alone", env, omega, base, allowed, None, None)
    run_and_compare(f"{tag} fixed alone", env, omega, start, None, fixed, None)
    run_and_compare(f"{tag} capacity alone, a negative and a zero one", env, omega, base, None, None,
                    np.where(capacity == 1, -1, capacity - 2).astype(np.int32))


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_without_constraints_it_is_k_search(shape, omega):
    """NULL constraints and neutral arrays (all ones, all zeros, capacity N) are each bitwise
    search_assignments on every output; max_exchanges = 0 with neutral arrays is refine_assignments."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    neutral = [dev(env, x) for x in neutral_constraints(N, M, E)]
    ids = random_starts(N, M, E)
    ids[0, 0] = M + 3  # an id of no target
    for start in (None, dev(env, ids)):
        plain = env.search_assignments(start)
        for con in ((None, None, None), (neutral[0], neutral[1], neutral[2])):
            got = env.search_assignments_constrained(start, *con)
            torch.cuda.synchronize()
            for x, y in zip(got[:3], plain[:3]):
                assert torch.equal(x, y), (shape, omega)
            assert torch.equal(got[3][:, :6], plain[3]) and not bool(got[3][:, 6:].any()), (shape, omega)
        refined = env.refine_assignments(start)
        zero = env.search_assignments_constrained(start, neutral[0], neutral[1], neutral[2], max_exchanges=0)
        torch.cuda.synchronize()
        for x, y in zip(zero[:3], refined[:3]):
            assert torch.equal(x, y), (shape, omega)
        assert torch.equal(zero[3][:, :4], refined[3]) and not bool(zero[3][:, 4:].any()), (shape, omega)


def test_cap_and_continuation():
    """max_exchanges = 1 at 16 x 32 stops the rows that need more with scan_clean = 0; feeding its
    output back with the same constraints ends on the one-call result, assignments and J bitwise,
    and drops nothing: the output of a call is feasible."""
    N, M, E, omega = 16, 32, 32, 0.0
    env = make_env(host_scenes(N, M, E), N, M, omega)
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    start, fixed = with_fixed(None, fixed_ids)
    full, got = run_and_compare("cap 32", env, omega, start, allowed, fixed, capacity)
    need = full[3][:, 4]
    assert need.max() >= 2 and need.min() <= 1, need
    one, first = run_and_compare("cap 1", env, omega, start, allowed, fixed, capacity, max_exchanges=1)
    assert np.array_equal(one[3][:, 4], np.minimum(need, 1))
    assert np.array_equal(one[3][:, 5], (need <= 1).astype(np.int32))
    second = env.search_assignments_constrained(first[0], dev(env, allowed), dev(env, fixed), dev(env, capacity),
                                                max_exchanges=31)
    torch.cuda.synchronize()
    assert torch.equal(second[0], got[0]) and torch.equal(second[1], got[1]) and torch.equal(second[2], got[2])
    st = second[3].cpu().numpy()
    assert np.array_equal(st[:, 4], need - np.minimum(need, 1)) and bool((st[:, 5] == 1).all())
    assert not st[:, 6].any() and np.array_equal(st[:, 7], full[3][:, 7])
    # no sweeps: the start, the scan alone, an exchange, no sweep after it
    start, fixed = with_fixed(random_starts(N, M, E), fixed_ids)
    run_and_compare("cap 3, no sweeps", env, omega, start, allowed, fixed, capacity, max_exchanges=3, max_sweeps=0)


def test_stride_rows_in_place_and_read_only():
    N, M, E, omega, K = 5, 7, 33, 0.5, 3
    dec = decoded_env(host_scenes(N, M, E), N, M, omega, K)
    names = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")
    before = {k: getattr(dec, k).clone() for k in names}
    before.update({"scene/" + k: t.clone() for k, t in dec._scene.items()})
    best, _, _, asg = dec.select_best(K)
    assert bool((best >= 0).all())
    allowed, capacity, fixed_ids = random_constraints(N, M, E)  # indexed by row, not by env
    start, fixed = with_fixed(asg.cpu().numpy(), fixed_ids)
    want, _ = run_and_compare("from best-of-3, stride 3", dec, omega, start, allowed, fixed, capacity, stride=K, rows=E)
    assert want[3][:, 6].sum() > 0
    run_and_compare("from best-of-3, stride 3, 7 rows", dec, omega, start[:7].copy(), allowed[:7].copy(),
                    fixed[:7].copy(), capacity[:7].copy(), stride=K, rows=7)
    con = [dev(dec, x) for x in (allowed, fixed, capacity)]
    kept = [x.clone() for x in con]
    buf = dev(dec, start)
    a, J, cov, st = dec.search_assignments_constrained(buf.clone(), *con, stride=K, rows=E)
    b, J2, cov2, st2 = dec.search_assignments_constrained(buf, *con, stride=K, rows=E, out=buf)
    torch.cuda.synchronize()
    assert b.data_ptr() == buf.data_ptr()
    for x, y in ((a, b), (J, J2), (cov, cov2), (st, st2)) + tuple(zip(con, kept)):
        assert torch.equal(x, y)
    for k in names:
        assert torch.equal(getattr(dec, k), before[k]), k
    for k, t in dec._scene.items():
        assert torch.equal(t, before["scene/" + k]), k


def _fields(r):
    return (r.assignment, r.J, r.covered, r.best_replica, r.steps, r.replica_J, r.decoded_J, r.refine_stats)


def test_through_the_solver():
    """solve(constraints=) is the direct call on select_best's output with the fixed ids written in, the
    decode untouched; baseline(constraints=) the direct call from the fixed ids alone; constraints = None
    is today's solve, bitwise."""
    from uavhip import AllocationSolver, Constraints
    N, M, S, K = 16, 32, 8, 2
    solver = AllocationSolver(gpu_policy(N, M, 1), N, M, samples=K)
    r0 = solver.solve(num_scenes=S, seed=5)
    for kw in (dict(refine=32), dict(refine=32, exchanges=32)):
        for x, y in zip(_fields(solver.solve(num_scenes=S, seed=5, **kw)),
                        _fields(solver.solve(num_scenes=S, seed=5, constraints=None, **kw))):
            assert torch.equal(x, y)
    allowed, capacity, fixed_ids = random_constraints(N, M, S)
    con = Constraints(allowed=torch.from_numpy(allowed), capacity=capacity, fixed_ids=torch.from_numpy(fixed_ids))
    for exchanges in (32, 0):
        rx = solver.solve(num_scenes=S, seed=5, refine=32, exchanges=exchanges, constraints=con)
        env = solver.env
        start, fixed = with_fixed(r0.assignment.cpu().numpy(), fixed_ids)
        alone = env.search_assignments_constrained(dev(env, start), dev(env, allowed), dev(env, fixed),
                                                   dev(env, capacity), stride=K, rows=S, max_exchanges=exchanges,
                                                   max_sweeps=32)
        torch.cuda.synchronize()
        for x, y in zip((rx.assignment, rx.J, rx.covered, rx.refine_stats), alone):
            assert torch.equal(x, y)
        assert rx.refine_stats.shape == (S, 8) and torch.equal(rx.decoded_J, r0.J)
        for x, y in zip(_fields(rx)[3:6], _fields(r0)[3:6]):
            assert torch.equal(x, y)
        check_guarantees(f"solve, exchanges {exchanges}", rx.assignment.cpu().numpy(), tables(env, K, S)[4], start,
                         allowed, fixed, capacity)
        print(f"solve 16 x 32, {S} scenes, K = {K}, exchanges {exchanges}: mean J decoded {r0.J.mean().item():.4f}, "
              f"constrained {rx.J.mean().item():.4f}, dropped {rx.refine_stats[:, 6].tolist()}")
    assert rx.cpu().refine_stats.shape == (S, 8)
    bx = solver.baseline(num_scenes=S, seed=5, exchanges=32, constraints=con)
    env = solver.env
    start, fixed = with_fixed(None, fixed_ids)
    alone = env.search_assignments_constrained(dev(env, start), dev(env, allowed), dev(env, fixed), dev(env, capacity),
                                               stride=K, rows=S)
    torch.cuda.synchronize()
    for x, y in zip((bx.assignment, bx.J, bx.covered, bx.refine_stats), alone):
        assert torch.equal(x, y)
    assert bx.decoded_J is None and bx.refine_stats.shape == (S, 8)
    # a constraint alone, and no committed UAV: the start is the empty one
    only = solver.baseline(num_scenes=S, seed=5, exchanges=32, constraints=Constraints(capacity=capacity))
    alone = solver.env.search_assignments_constrained(None, None, None, dev(env, capacity), stride=K, rows=S)
    torch.cuda.synchronize()
    for x, y in zip((only.assignment, only.J, only.covered, only.refine_stats), alone):
        assert torch.equal(x, y)
