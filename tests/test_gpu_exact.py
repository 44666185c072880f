"""uavhip_solve_exact on the GPU (k_exact_prepare / k_exact_stage / k_exact_backtrack): the kernels'
J against exact_np, the numpy subset DP of tests/test_exact_host.py, fed the pair tables read back from
the device; and, on the kernels' own outputs, J bitwise refine_assignments(out, max_sweeps=0)'s, the
guarantees of the constrained search, stats, two launches bitwise equal, and a workspace of 2 rows for
5 rows. At 16 x 32, where no numpy DP is affordable: never below the searches, above the search in the
row the CPU found, unchanged under a reordering of the scene; and AllocationSolver.optimum.

Shapes (N, M, E): one bit (1 x 3); 4 x 4; 5 x 7 with 33 rows (a partial last workgroup of the one-wave-
per-row kernels); 9 x 12, just past a byte; 11 x 66, one high bit above the tile's ten and two targets
per lane in the one-wave-per-row kernels; 16 x 3, the full 16-bit set with six high bits."""
import numpy as np
import pytest
import torch

import capi_host
from test_constrained_search_host import check_guarantees, random_constraints, with_fixed
from test_exact_host import exact_rows, exact_stats
from test_gpu_refine import make_env, tables
from test_gpu_solve import gpu_policy
from test_refine_host import OMEGAS, RTOL_J, host_scenes, random_starts

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 2), (4, 4, 6), (5, 7, 33), (9, 12, 5), (11, 66, 2), (16, 3, 2)]

_entry_point = capi_host._entry_point("uavhip_solve_exact")


def dev(env, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(env.device)


def bar(J):
    return RTOL_J * np.maximum(1.0, np.abs(J))


def launch(env, start=None, allowed=None, fixed=None, capacity=None, **kw):
    got = env.exact_assignments(dev(env, start), dev(env, allowed), dev(env, fixed), dev(env, capacity), **kw)
    torch.cuda.synchronize()
    return got


def check_own_outputs(label, env, got, start, allowed, fixed, capacity, stride=1, rows=None):
    """What the header promises of the outputs themselves."""
    asg, J, cov, st = got
    scored = env.refine_assignments(asg, stride=stride, rows=rows, max_sweeps=0)
    torch.cuda.synchronize()
    assert asg.dtype == torch.int32 and torch.equal(scored[0], asg), label
    assert torch.equal(scored[1], J) and torch.equal(scored[2], cov), label        # bitwise
    ids = tables(env, stride, rows)[4]
    check_guarantees(label, asg.cpu().numpy(), ids, start, allowed, fixed, capacity)
    assert st.shape == (len(J), 2) and np.array_equal(st.cpu().numpy(), exact_stats(ids, start, allowed, fixed, capacity)), label


def run_and_compare(label, env, omega, start=None, allowed=None, fixed=None, capacity=None, want=None):
    """One launch against exact_np on the device's tables (want: its J where a caller has them already);
    a second launch bitwise equal. Returns (the launch's outputs, exact_np's J)."""
    got = launch(env, start, allowed, fixed, capacity)
    if want is None:
        _, want = exact_rows(*tables(env), omega, start, allowed, fixed, capacity)
    J = got[1].cpu().numpy()
    err = np.abs(J - want) / np.maximum(1.0, np.abs(want))
    print(f"{label}: {len(J)} rows, mean J {want.mean():.6f}, max J err {err.max():.2e} (bar {RTOL_J:g}), "
          f"stats sum {got[3].sum(0).tolist()}")
    assert bool((err <= RTOL_J).all()), (label, float(err.max()))
    check_own_outputs(label, env, got, start, allowed, fixed, capacity)
    again = launch(env, start, allowed, fixed, capacity)
    for x, y in zip(got, again):
        assert torch.equal(x, y), label
    return got, want


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_reaches_the_numpy_optimum(shape, omega):
    """Unconstrained and under seeded constraints (mask density 0.7, capacities in {1, 2, 3}, a fifth of
    the UAVs committed), from the empty start and with the committed UAVs written into random ids; a
    negative and a zero capacity; a UAV fixed to none and one fixed to an id of no target."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    tag = f"({N}, {M}, {E}) omega {omega}"
    free, _ = run_and_compare(f"{tag} unconstrained", env, omega)
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    want = None  # a free UAV's start is not looked at: both starts have one feasible set, one optimum
    for name, base in (("empty", None), ("random ids", random_starts(N, M, E))):
        start, fixed = with_fixed(base, fixed_ids)
        got, want = run_and_compare(f"{tag} constrained from {name}", env, omega, start, allowed, fixed, capacity, want)
        assert bool((got[1].cpu().numpy() <= free[1].cpu().numpy() + bar(free[1].cpu().numpy())).all()), tag
    loose = launch(env, random_starts(N, M, E), None, None, None)
    assert torch.equal(loose[0], free[0]) and torch.equal(loose[1], free[1])
    if N == 16:
        return  # the cases below are about the masks, not the tiling: the numpy DP's seconds go to the shapes above
    run_and_compare(f"{tag} a negative and a zero capacity", env, omega, None, None, None,
                    np.where(capacity == 1, -1, capacity - 2).astype(np.int32))
    odd, odd_fixed = start.copy(), np.zeros_like(fixed)
    odd[:, 0], odd_fixed[:, 0] = -1, 1
    if N > 1:
        odd[:, 1], odd_fixed[:, 1] = M + 3, 1
    got, _ = run_and_compare(f"{tag} fixed to none and to an invalid id", env, omega, odd, allowed, odd_fixed, capacity)
    assert bool((got[0][:, :min(N, 2)] == -1).all()) and bool((got[3][:, 0] >= min(N, 2) - 1).all())


def test_chunks_stride_rows_and_read_only():
    """A workspace for 2 of 5 rows gives the outputs of a workspace for all; stride and rows pick the
    scenes refine_assignments picks; the env and the inputs are only read; caller buffers are used."""
    N, M, E, omega = 9, 12, 5, 0.5
    env = make_env(host_scenes(N, M, E), N, M, omega)
    from uavhip import _lib
    row = int(_lib.LIB.uavhip_exact_workspace_bytes(N, M, 1))
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    start, fixed = with_fixed(random_starts(N, M, E), fixed_ids)
    names = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")
    before = {k: getattr(env, k).clone() for k in names}
    before.update({"scene/" + k: t.clone() for k, t in env._scene.items()})
    whole = launch(env, start, allowed, fixed, capacity)
    for nbytes in (2 * row, 3 * row - 1, row):
        part = launch(env, start, allowed, fixed, capacity, max_workspace_bytes=nbytes)
        for x, y in zip(whole, part):
            assert torch.equal(x, y), nbytes
    con = [dev(env, x) for x in (start, allowed, fixed, capacity)]
    kept = [x.clone() for x in con]
    bufs = dict(out=torch.empty(E, N, dtype=torch.int32, device=env.device),
                J=torch.empty(E, dtype=torch.float64, device=env.device),
                covered=torch.empty(E, dtype=torch.int32, device=env.device),
                stats=torch.empty(E, 2, dtype=torch.int32, device=env.device))
    mine = env.exact_assignments(*con, **bufs)
    torch.cuda.synchronize()
    for x, y, z in zip(mine, whole, bufs.values()):
        assert x.data_ptr() == z.data_ptr() and torch.equal(x, y)
    for x, y in zip(con, kept):
        assert torch.equal(x, y)
    for k in names:
        assert torch.equal(getattr(env, k), before[k]), k
    for k, t in env._scene.items():
        assert torch.equal(t, before["scene/" + k]), k
    # rows 0, 2, 4 of the scenes at stride 2: the constraint arrays are indexed by row
    strided = launch(env, start[:3].copy(), allowed[:3].copy(), fixed[:3].copy(), capacity[:3].copy(), stride=2, rows=3)
    _, want = exact_rows(*tables(env, 2, 3), omega, start[:3], allowed[:3], fixed[:3], capacity[:3])
    J = strided[1].cpu().numpy()
    assert bool((np.abs(J - want) <= bar(want)).all())
    check_own_outputs("stride 2", env, strided, start[:3], allowed[:3], fixed[:3], capacity[:3], stride=2, rows=3)
    two = launch(env, start[:2].copy(), allowed[:2].copy(), fixed[:2].copy(), capacity[:2].copy(), rows=2)
    for x, y in zip(two, whole):
        assert torch.equal(x, y[:2])


def reordered(scene, uavs=False, targets=False):
    """The same scene with its UAVs and / or its targets listed in reversed order."""
    out = dict(scene)
    for k, v in scene.items():
        if uavs and k.startswith("uav_"):
            out[k] = np.ascontiguousarray(np.asarray(v)[::-1])
        if targets and k.startswith("tgt_"):
            out[k] = np.ascontiguousarray(np.asarray(v)[::-1])
    return out


@pytest.fixture(scope="module")
def headline():
    """(16, 32, 4) at both omegas: env, the optimum's outputs, the search's."""
    N, M, E = 16, 32, 4
    out = {}
    for omega in OMEGAS:
        env = make_env(host_scenes(N, M, E), N, M, omega)
        best = launch(env)
        found = env.search_assignments(None)
        torch.cuda.synchronize()
        out[omega] = (env, best, found)
    return out


@pytest.mark.parametrize("omega", OMEGAS)
def test_headline_shape_against_the_searches(headline, omega):
    """16 x 32: the optimum is never below the exchange search in any row, nor below the constrained
    search under constraints; at omega = 0, row 0 exceeds the search by more than 1e-3 (a 16-thread CPU
    DP gives 33.8985 against the search's 33.7308 on the oracle's tables)."""
    N, M, E = 16, 32, 4
    env, best, found = headline[omega]
    J, Js = best[1].cpu().numpy(), found[1].cpu().numpy()
    print(f"omega {omega}: optimum {J.tolist()}, search {Js.tolist()}")
    assert bool((J >= Js - bar(J)).all())
    check_own_outputs(f"16 x 32 omega {omega}", env, best, None, None, None, None)
    if omega == 0.0:
        assert J[0] > Js[0] + 1e-3
        assert abs(J[0] - 33.8985) < 1e-3 and abs(Js[0] - 33.7308) < 1e-3
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    start, fixed = with_fixed(None, fixed_ids)
    got = launch(env, start, allowed, fixed, capacity)
    local = env.search_assignments_constrained(dev(env, start), dev(env, allowed), dev(env, fixed), dev(env, capacity))
    torch.cuda.synchronize()
    Jc, Jl = got[1].cpu().numpy(), local[1].cpu().numpy()
    print(f"omega {omega} constrained: optimum {Jc.tolist()}, search {Jl.tolist()}")
    assert bool((Jc >= Jl - bar(Jc)).all()) and bool((Jc <= J + bar(J)).all())
    check_own_outputs(f"16 x 32 omega {omega} constrained", env, got, start, allowed, fixed, capacity)
    again = launch(env, start, allowed, fixed, capacity)
    for x, y in zip(got, again):
        assert torch.equal(x, y)


@pytest.mark.parametrize("omega", OMEGAS)
def test_headline_shape_under_reordering(headline, omega):
    """The optimum is a property of the scene: unchanged to the reward bar with the UAVs loaded in
    reversed order, and with the targets."""
    N, M, E = 16, 32, 4
    J = headline[omega][1][1].cpu().numpy()
    for kw in (dict(uavs=True), dict(targets=True)):
        env = make_env(tuple(reordered(s, **kw) for s in host_scenes(N, M, E)), N, M, omega)
        Jr = launch(env)[1].cpu().numpy()
        assert bool((np.abs(Jr - J) <= bar(J)).all()), (kw, J, Jr)


def test_through_the_solver():
    """AllocationSolver.optimum is the direct call on the same scenes, with and without constraints, and
    baseline() never exceeds it."""
    from uavhip import AllocationSolver, Constraints
    N, M, S, K = 16, 32, 4, 2
    solver = AllocationSolver(gpu_policy(N, M, 1), N, M, samples=K)
    allowed, capacity, fixed_ids = random_constraints(N, M, S)
    con = Constraints(allowed=torch.from_numpy(allowed), capacity=capacity, fixed_ids=torch.from_numpy(fixed_ids))
    for c in (None, con):
        opt = solver.optimum(num_scenes=S, seed=5, constraints=c)
        env = solver.env
        start, fixed = (None, None) if c is None else with_fixed(None, fixed_ids)
        alone = launch(env, start, None if c is None else allowed, fixed, None if c is None else capacity, stride=K, rows=S)
        for x, y in zip((opt.assignment, opt.J, opt.covered, opt.refine_stats), alone):
            assert torch.equal(x, y)
        assert opt.decoded_J is None and opt.refine_stats.shape == (S, 2) and opt.replica_J.shape == (S, K)
        assert not bool(opt.best_replica.any()) and not bool(opt.steps.any())
        for exchanges in (0, 32):
            base = solver.baseline(num_scenes=S, seed=5, exchanges=exchanges, constraints=c)
            assert bool((base.J <= opt.J + RTOL_J * opt.J.abs().clamp(min=1.0)).all()), (c is None, exchanges)
        print(f"16 x 32, {S} scenes, constraints {c is not None}: optimum {opt.J.tolist()}, baseline {base.J.tolist()}")
    hosts = list(host_scenes(N, M, 2))
    a, b = solver.optimum(scenes=hosts), solver.optimum(scenes=hosts, max_workspace_bytes=6 << 20)
    assert torch.equal(a.J, b.J) and torch.equal(a.assignment, b.assignment)
