"""uavhip_search_multistart_from on the GPU (k_search_multistart / k_multistart_select with R0 given
starts per row). Launch against launch every comparison is bitwise: R0 = 1 is the existing multi-start
in all five outputs; a given replica's J is search_assignments_constrained's from that replica's start
(the fixed UAVs' ids taken from start 0); a random replica's J is the existing multi-start's at the same
r, s and seed; the chosen replica is the lowest argmax of the device's own J_all and its assignment,
covered and eight counters are that replica's own single launch. Against multistart_from_np, the Python
restatement (tests/test_policy_starts_host.py) fed the pair tables read back from the device: the
chosen replica's assignment, covered and counters exactly, and every replica's J to the project's reward
bar RTOL_J = 1e-12 max(1, |J|) -- the restatement adds the targets' terms in list order, the kernel in a
butterfly, so their J differ in the last bits; that is the bar tests/test_gpu_multistart.py holds the
sibling to, and no comparison between two launches uses it. Then the constraints' guarantees,
determinism, stride and rows, read-only inputs, AllocationSolver.solve(starts="replicas") and the optimum.

Shapes (N, M, E), the smallest that reach each instantiation and both lane layouts: (5, 7, 33) <1, 8>,
(16, 32, 32) <1, 16>, (20, 24, 3) <1, 32>, (33, 34, 3) <1, 0>, (12, 70, 5) <2, 0>. R = 6, R0 in
{1, 3, 6}, caps 32 / 32."""
import numpy as np
import pytest
import torch

import capi_host
from test_constrained_search_host import check_guarantees
from test_gpu_multistart import _fields, bar, dev
from test_gpu_multistart import launch as launch_sibling
from test_gpu_refine import decoded_env, make_env, tables
from test_gpu_solve import gpu_policy
from test_multistart_host import random_start
from test_policy_starts_host import given_starts, multistart_from_rows
from test_refine_host import OMEGAS, RTOL_J, host_scenes

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 33), (16, 32, 32), (20, 24, 3), (33, 34, 3), (12, 70, 5)]
R, R0S, SEED = 6, (1, 3, 6), (7 << 32) + 3
FIXED_UAVS = (1, 3)

_entry_point = capi_host._entry_point("uavhip_search_multistart_from")


def launch(env, R, starts, seed=SEED, allowed=None, fixed=None, capacity=None, stride=1, rows=None, **kw):
    """-> (assignment, J, covered, stats, J_all) device tensors of one call from `starts` [rows, R0, N]."""
    S = len(starts)
    J_all = torch.full((S, R), float("nan"), dtype=torch.float64, device=env.device)
    got = env.search_assignments_multistart(None, dev(env, allowed), dev(env, fixed), dev(env, capacity), restarts=R,
                                            seed=seed, stride=stride, rows=rows, J_all=J_all, starts=dev(env, starts), **kw)
    torch.cuda.synchronize()
    return got + (J_all,)


def starts_for(env, N, M, S, stride=1):
    """[S, R, N]: start 0 empty, start 1 one sweep of the best-response search from nothing, the others
    given_starts' random ids (some -1, an id of no target on UAV 0, UAVs 1 and 2 on the same id)."""
    a = given_starts(N, M, S, R)
    a[:, 1] = env.refine_assignments(None, stride=stride, rows=S, max_sweeps=1)[0].cpu().numpy()
    return a


def constraints_for(N, M, S, starts, seed=13):
    """A fifth of the pairs forbidden, capacity 1 on a quarter of the targets (else no limit), UAVs 1 and
    3 fixed, on ids that differ between start 0 and start 1. -> (starts, allowed, fixed, capacity)."""
    rng = np.random.default_rng(seed)
    allowed = (rng.random((S, N, M)) >= 0.2).astype(np.uint8)
    capacity = np.where(rng.random((S, M)) < 0.25, 1, N).astype(np.int32)
    fixed = np.zeros((S, N), np.uint8)
    starts = starts.copy()
    for i, u in enumerate(FIXED_UAVS):
        fixed[:, u] = 1
        starts[:, 0, u] = (np.arange(S) + 2 * i) % M
        starts[:, 1, u] = (starts[:, 0, u] + 1) % M
    starts[::4, 0, FIXED_UAVS[1]] = -1  # fixed to none in every fourth row
    return starts, allowed, fixed, capacity


def own_start(starts, fixed, r):
    """What replica r < R0 is given: start r with start 0's ids on the fixed UAVs."""
    if fixed is None or r == 0:
        return np.ascontiguousarray(starts[:, r])
    return np.where(fixed != 0, starts[:, 0], starts[:, r]).astype(np.int32)


def single_launches(env, tgt_id, starts, seed, con, stride=1, rows=None):
    """search_assignments_constrained once per start a replica r < R can have: given, from own_start (r <
    len(starts[0])), and drawn, from the ids of the random list indices (r >= 1; the ids of a scene are
    distinct, so they convert back) with start 0's ids on the fixed UAVs.
    -> (given, drawn): per replica (assignment, J, covered, stats) as numpy; drawn[0] is given[0]."""
    S, R0, N = starts.shape
    M = tgt_id.shape[1]

    def run(start):
        got = env.search_assignments_constrained(dev(env, start), *(dev(env, x) for x in con), stride=stride, rows=rows)
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in got)
    given = [run(own_start(starts, con[1], r)) for r in range(R0)]
    drawn = [given[0]]
    for r in range(1, R):
        idx = np.array([random_start(N, M, r, s, seed) for s in range(S)])
        start = np.take_along_axis(tgt_id, idx, 1).astype(np.int32)
        if con[1] is not None:
            start = np.where(con[1] != 0, starts[:, 0], start).astype(np.int32)
        drawn.append(run(start))
    return given, drawn


def check_against_launches(label, got, singles, sibling_J_all, R0):
    """The header's rule on the call's outputs, every comparison bitwise."""
    asg, J, cov, st, J_all = (t.cpu().numpy() for t in got)
    S = len(J)
    singles = singles[0][:R0] + singles[1][R0:]
    assert st.shape == (S, 10) and asg.dtype == np.int32 and not np.isnan(J_all).any(), label
    for r in range(R):
        want = singles[r][1] if r < R0 else sibling_J_all[:, r]
        assert np.array_equal(J_all[:, r], want), (label, r)
        assert np.array_equal(J_all[:, r], singles[r][1]), (label, r)  # a random replica too is its own single launch
    assert np.array_equal(J, J_all.max(1)), label
    assert np.array_equal(st[:, 8], np.argmax(J_all, 1)), label  # the lowest index attaining it
    assert np.array_equal(st[:, 9], (J_all > J_all[:, :1]).sum(1)), label
    for s in range(S):
        w = int(st[s, 8])
        a1, _, c1, s1 = singles[w]
        assert np.array_equal(asg[s], a1[s]) and cov[s] == c1[s], (label, s, w)
        invalid = s1[s, 3] if w < R0 else singles[0][3][s, 3]  # a random replica converts all of start 0
        assert np.array_equal(st[s, :3], s1[s, :3]) and st[s, 3] == invalid and np.array_equal(st[s, 4:8], s1[s, 4:8]), \
            (label, s, w)


def restated(tabs, omega, starts, con, seed=SEED):
    """multistart_from_rows' replicas per row for R0 = R (every given replica) and R0 = 1 (every random
    one): a replica depends on r alone, so the rule for any R0 is the first R0 of the one and the rest of
    the other (tests/test_policy_starts_host.py checks that of the restatement)."""
    given = multistart_from_rows(*tabs, omega, R, R, seed, starts, *con)[3]
    drawn = multistart_from_rows(*tabs, omega, R, 1, seed, starts[:, :1], *con)[3]
    return given, drawn


def check_against_restatement(label, got, reps, R0):
    asg, J, cov, st, J_all = (t.cpu().numpy() for t in got)
    given, drawn = reps
    for s in range(len(J)):
        row = given[s][:R0] + drawn[s][R0:]
        want = np.array([x[1] for x in row])
        err = np.abs(J_all[s] - want) / np.maximum(1.0, np.abs(want))
        assert bool((err <= RTOL_J).all()), (label, s, float(err.max()))
        w = row[st[s, 8]]
        assert np.array_equal(asg[s], w[0]) and cov[s] == w[2] and np.array_equal(st[s, :8], w[3]), (label, s)


def assert_same(x, y, label=None):
    for a, b in zip(x, y):
        assert torch.equal(a, b), label


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_given_starts_against_launches_and_restatement(shape, omega):
    """Unconstrained, every R0: R0 = 1 is the existing call in all five outputs; then the rule launch
    against launch and against multistart_from_np."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    starts = starts_for(env, N, M, E)
    con = (None, None, None)
    tabs = tables(env)
    sibling = launch_sibling(env, R, SEED, np.ascontiguousarray(starts[:, 0]))
    assert_same(launch(env, R, starts[:, :1]), sibling, (shape, omega))
    singles = single_launches(env, tabs[4], starts, SEED, con)
    reps = restated(tabs, omega, starts, con)
    for R0 in R0S:
        label = f"{shape} omega {omega} R0 = {R0}"
        got = launch(env, R, starts[:, :R0])
        check_against_launches(label, got, singles, sibling[4].cpu().numpy(), R0)
        check_against_restatement(label, got, reps, R0)
        print(f"{label}: mean J {got[1].mean().item():.6f}, chosen {got[3][:, 8].tolist()}")
    six = launch(env, R, starts)[3].cpu().numpy()
    for s in range(E):  # the id of no target is counted in the replicas that were given it
        assert six[s, 3] == (1 if six[s, 8] >= 2 else 0), (shape, omega, s)


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", [(5, 7, 33), (16, 32, 32)])
def test_under_constraints(shape, omega):
    """constraints_for's arrays: the fixed UAVs leave where start 0 put them whichever replica wins, the
    constrained search's guarantees hold for the output, every given replica is the constrained search
    from own_start bitwise, and the restatement agrees."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    starts, allowed, fixed, capacity = constraints_for(N, M, E, starts_for(env, N, M, E))
    con = (allowed, fixed, capacity)
    tabs = tables(env)
    sibling = launch_sibling(env, R, SEED, np.ascontiguousarray(starts[:, 0]), *con)
    assert_same(launch(env, R, starts[:, :1], SEED, *con), sibling, (shape, omega))
    singles = single_launches(env, tabs[4], starts, SEED, con)
    reps = restated(tabs, omega, starts, con)
    won = set()
    for R0 in R0S:
        label = f"{shape} omega {omega} constrained R0 = {R0}"
        got = launch(env, R, starts[:, :R0], SEED, *con)
        check_against_launches(label, got, singles, sibling[4].cpu().numpy(), R0)
        check_against_restatement(label, got, reps, R0)
        asg = got[0].cpu().numpy()
        check_guarantees(label, asg, tabs[4], np.ascontiguousarray(starts[:, 0]), *con)  # fixed UAVs: start 0's ids
        for u in FIXED_UAVS:
            assert np.array_equal(asg[:, u], starts[:, 0, u]), (label, u)
        won |= set(got[3][:, 8].tolist())
    assert len(won) > 1  # not every row is won by replica 0: a replica whose own start disagreed on the fixed UAVs won


def test_determinism_stride_rows_and_read_only():
    N, M, E, omega, K = 5, 7, 33, 0.5, 3
    env = decoded_env(host_scenes(N, M, E), N, M, omega, K)
    names = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")
    before = {k: getattr(env, k).clone() for k in names}
    before.update({"scene/" + k: t.clone() for k, t in env._scene.items()})
    starts, allowed, fixed, capacity = constraints_for(N, M, E, starts_for(env, N, M, E, stride=K))  # indexed by row
    con = (allowed, fixed, capacity)
    tabs = tables(env, K, E)
    first = launch(env, R, starts[:, :3], SEED, *con, stride=K, rows=E)
    assert_same(first, launch(env, R, starts[:, :3], SEED, *con, stride=K, rows=E))   # the same seed: bitwise the same
    check_against_launches("stride 3", first, single_launches(env, tabs[4], starts[:, :3], SEED, con, K, E),
                           launch_sibling(env, R, SEED, np.ascontiguousarray(starts[:, 0]), *con, stride=K, rows=E)[4]
                           .cpu().numpy(), 3)
    check_against_restatement("stride 3", first, restated(tabs, omega, starts, con), 3)
    other = launch(env, R, starts[:, :3], SEED + 1, *con, stride=K, rows=E)
    assert torch.equal(other[4][:, :3], first[4][:, :3]) and not torch.equal(other[4], first[4])  # given replicas: no seed
    seven = launch(env, R, np.ascontiguousarray(starts[:7, :3]), SEED, *(x[:7].copy() for x in con), stride=K, rows=7)
    assert_same(seven, [t[:7] for t in first])
    given = dev(env, np.ascontiguousarray(starts[:, :3]))
    kept = given.clone()
    cons = [dev(env, x) for x in con]
    kept_cons = [x.clone() for x in cons]
    got = env.search_assignments_multistart(None, *cons, restarts=R, seed=SEED, stride=K, rows=E, starts=given)
    torch.cuda.synchronize()
    assert_same(got, first[:4])
    assert torch.equal(given, kept)
    assert_same(cons, kept_cons)
    for k in names:
        assert torch.equal(getattr(env, k), before[k]), k
    for k, t in env._scene.items():
        assert torch.equal(t, before["scene/" + k]), k


@pytest.mark.parametrize("N,M", [(5, 7), (16, 32)])
def test_through_the_solver(N, M):
    """solve(restarts=4, starts="replicas") is the hand-built decode -> assigned_target_ids ->
    search_assignments_multistart(starts=); never below solve(restarts=0), one of whose replicas it runs;
    once more with a committed UAV; starts="best" is the call without the argument."""
    from uavhip import AllocationSolver, Constraints
    S, K, Rs = 8, 4, 4
    solver = AllocationSolver(gpu_policy(N, M, 1), N, M, samples=K)
    kw = dict(num_scenes=S, seed=5, refine=32, exchanges=32)
    fixed_ids = torch.full((S, N), -2, dtype=torch.int32)
    fixed_ids[:, 2] = torch.arange(S, dtype=torch.int32) % M
    fixed_ids[0, 2] = -1
    for con in (None, Constraints(fixed_ids=fixed_ids)):
        today = solver.solve(constraints=con, **kw)
        for restarts in (0, 4):
            assert_same([x for x in _fields(solver.solve(constraints=con, restarts=restarts, **kw)) if x is not None],
                        [x for x in _fields(solver.solve(constraints=con, restarts=restarts, starts="best", **kw))
                         if x is not None])
        assert solver.solve(constraints=con, restarts=4, **kw).start_J is None and today.start_J is None
        rx = solver.solve(constraints=con, restarts=Rs, starts="replicas", **kw)
        env = solver.env
        given = env.assigned_target_ids().to(torch.int32).view(S, K, N).contiguous()
        fixed = None
        if con is not None:
            fx = fixed_ids.to(env.device)
            given = torch.where(fx.view(S, 1, N) != -2, fx.view(S, 1, N), given).contiguous()
            fixed = (fx != -2).to(torch.uint8)
        J_all = torch.empty(S, Rs, dtype=torch.float64, device=env.device)
        alone = env.search_assignments_multistart(None, None, fixed, None, restarts=Rs, seed=5, stride=K, rows=S,
                                                  J_all=J_all, starts=given)
        torch.cuda.synchronize()
        assert_same((rx.assignment, rx.J, rx.covered, rx.refine_stats, rx.start_J), alone + (J_all,))
        assert rx.refine_stats.shape == (S, 10) and rx.start_J.shape == (S, Rs) and rx.cpu().start_J.shape == (S, Rs)
        assert_same((rx.decoded_J, rx.best_replica, rx.replica_J, rx.steps),
                    (today.decoded_J, today.best_replica, today.replica_J, today.steps))
        assert bool((rx.best_replica >= 0).all())
        J, J0 = rx.J.cpu().numpy(), today.J.cpu().numpy()
        assert J.dtype == np.float64 and bool((J >= J0).all()), (J, J0)
        picked = torch.gather(rx.start_J, 1, rx.best_replica.long().view(S, 1)).view(S)
        assert torch.equal(picked, today.J)  # the polish of restarts = 0 is replica best_replica of the search
        print(f"{N} x {M}, {S} scenes, constraints {con is not None}: mean J {J0.mean():.4f} -> {J.mean():.4f}, "
              f"chosen {rx.refine_stats[:, 8].tolist()}, best decoded replica {rx.best_replica.tolist()}")
        if con is not None:
            ids = tables(env, K, S)[4]
            start = torch.where(fx != -2, fx, given[:, 0]).cpu().numpy()
            check_guarantees("solve, replicas, committed UAV", rx.assignment.cpu().numpy(), ids, start, None,
                             fixed.cpu().numpy(), None)


@pytest.mark.parametrize("omega", OMEGAS)
def test_never_above_the_optimum(omega):
    """(16, 32, 8): J <= exact_assignments' J + the bar in every row and every replica, at every R0."""
    N, M, E = 16, 32, 8
    env = make_env(host_scenes(N, M, E), N, M, omega)
    starts = starts_for(env, N, M, E)
    best = env.exact_assignments()
    torch.cuda.synchronize()
    Jx = best[1].cpu().numpy()
    for R0 in R0S:
        got = launch(env, R, starts[:, :R0])
        J = got[1].cpu().numpy()
        print(f"omega {omega}, R0 = {R0}: share of the optimum {J.mean() / Jx.mean():.5f}, "
              f"{int((J >= Jx - bar(Jx)).sum())} of {E} rows optimal")
        assert bool((J <= Jx + bar(Jx)).all()), (J, Jx)
        assert bool((got[4].cpu().numpy() <= Jx[:, None] + bar(Jx)[:, None]).all())
