"""uavhip_search_multistart on the GPU (k_search_multistart / k_multistart_select): the kernels against
multistart_np, the Python restatement of the rule (tests/test_multistart_host.py), fed the pair tables
read back from the device -- every replica's J to the project's reward bar; on the device's own J_all
the choice of the replica bit for bit; the chosen replica's assignment, covered and eight counters
exactly -- replica 0 bitwise the constrained search; the improvement a CPU run of the rule found at
16 x 32; the constraints' guarantees; never above the exact optimum; determinism, stride, rows, in place;
and the layers above: AllocationSolver.solve / baseline(restarts=) and the command line.

Shapes (N, M, E): the register-column path at its three capacities (4 x 4 and 5 x 7: 8; 16 x 32: 16;
17 x 20: 32), the streamed path (33 x 34) and two targets per lane (12 x 70, 8 x 128) -- all five
instantiations. R = 5 leaves S * R off a multiple of the workgroup's four waves at every odd E."""
import json

import numpy as np
import pytest
import torch

import capi_host
from test_constrained_search_host import check_guarantees, random_constraints, with_fixed
from test_gpu_refine import decoded_env, make_env, tables
from test_gpu_solve import gpu_policy
from test_multistart_host import multistart_rows
from test_refine_host import OMEGAS, RTOL_J, host_scenes, random_starts

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4, 6), (5, 7, 33), (16, 32, 32), (17, 20, 5), (33, 34, 3), (12, 70, 5), (8, 128, 3)]
SIXTEEN = [(16, 32, 32), (33, 34, 3)]  # the shapes that also run R = 16

_entry_point = capi_host._entry_point("uavhip_search_multistart")


def dev(env, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(env.device)


def bar(J):
    return RTOL_J * np.maximum(1.0, np.abs(J))


def launch(env, R, seed=0, start=None, allowed=None, fixed=None, capacity=None, stride=1, rows=None, **kw):
    """-> (assignment, J, covered, stats, J_all) device tensors of one call."""
    S = (env.E - 1) // stride + 1 if rows is None else rows
    J_all = torch.full((S, R), float("nan"), dtype=torch.float64, device=env.device)
    got = env.search_assignments_multistart(dev(env, start), dev(env, allowed), dev(env, fixed), dev(env, capacity),
                                            restarts=R, seed=seed, stride=stride, rows=rows, J_all=J_all, **kw)
    torch.cuda.synchronize()
    return got + (J_all,)


def check_choice(label, got):
    """What the header says of the outputs, on the device's own J_all."""
    asg, J, cov, st, J_all = (t.cpu().numpy() for t in got)
    S, R = J_all.shape
    assert st.shape == (S, 10) and asg.dtype == np.int32, label
    assert not np.isnan(J_all).any(), label
    assert np.array_equal(J, J_all.max(1)), label                                   # bitwise
    assert np.array_equal(st[:, 8], np.argmax(J_all, 1)), label                     # the lowest index attaining it
    assert np.array_equal(st[:, 9], (J_all > J_all[:, :1]).sum(1)), label


def run_and_compare(label, env, omega, R, seed=0, start=None, allowed=None, fixed=None, capacity=None, stride=1,
                    rows=None):
    """One call against multistart_np on the device's tables. Returns the call's outputs."""
    got = launch(env, R, seed, start, allowed, fixed, capacity, stride, rows)
    asg, J, cov, st, J_all = (t.cpu().numpy() for t in got)
    tabs = tables(env, stride, rows)
    want_J, _, _, reps = multistart_rows(*tabs, omega, R, seed, start, allowed, fixed, capacity)
    err = np.abs(J_all - want_J) / np.maximum(1.0, np.abs(want_J))
    print(f"{label}: {len(J)} rows x {R}, mean J {want_J[:, 0].mean():.6f} -> {J.mean():.6f}, chosen {st[:, 8].tolist()}, "
          f"above replica 0 {st[:, 9].tolist()}, max J err {err.max():.2e} (bar {RTOL_J:g})")
    assert bool((err <= RTOL_J).all()), (label, float(err.max()))
    check_choice(label, got)
    for s in range(len(J)):
        w = reps[s][st[s, 8]]
        assert np.array_equal(asg[s], w[0]) and cov[s] == w[2] and np.array_equal(st[s, :8], w[3]), (label, s)
    check_guarantees(label, asg, tabs[4], start, allowed, fixed, capacity)
    return got


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_are_the_restatement(shape, omega):
    """Unconstrained: R = 1 and 5 from the empty start (16 where SIXTEEN says so), R = 5 from random ids
    with an id of no target among them."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    tag = f"({N}, {M}, {E}) omega {omega}"
    for R in (1, 5) + ((16,) if shape in SIXTEEN else ()):
        run_and_compare(f"{tag} R = {R} from empty", env, omega, R)
    ids = random_starts(N, M, E)
    ids[0, 0] = M + 3
    got = run_and_compare(f"{tag} R = 5 from random ids", env, omega, 5, seed=(7 << 32) + 3, start=ids)
    assert int(got[3][0, 3]) == 1  # the invalid id is counted whichever replica wins


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_one_replica_is_the_constrained_search(shape, omega):
    """R = 1 is search_assignments_constrained bitwise in all four outputs, with constraints and
    without; without them also search_assignments on stats columns 0-5. Replica 0 of R = 5 likewise."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    start, fixed = with_fixed(random_starts(N, M, E), fixed_ids)
    for con in ((None, None, None, None), (random_starts(N, M, E), None, None, None), (start, allowed, fixed, capacity)):
        one = launch(env, 1, 4, *con)
        single = env.search_assignments_constrained(*(dev(env, x) for x in con))
        torch.cuda.synchronize()
        for x, y in zip(one[:3], single[:3]):
            assert torch.equal(x, y), (shape, omega)
        assert torch.equal(one[3][:, :8], single[3]) and not bool(one[3][:, 8:].any()), (shape, omega)
        assert torch.equal(one[4][:, 0], single[1])
        five = launch(env, 5, 4, *con)
        assert torch.equal(five[4][:, 0], single[1]), (shape, omega)
        if con[1] is None:
            plain = env.search_assignments(dev(env, con[0]))
            torch.cuda.synchronize()
            for x, y in zip(one[:3], plain[:3]):
                assert torch.equal(x, y), (shape, omega)
            assert torch.equal(one[3][:, :6], plain[3]), (shape, omega)


@pytest.mark.parametrize("omega", OMEGAS)
def test_restarts_improve_the_headline_shape(omega):
    """(16, 32, 32), R = 16, seed 0: at least 8 rows strictly above the single search, none below (a CPU
    run of the rule on the oracle's tables: 13 rows at omega = 0, 11 at 0.5)."""
    N, M, E = 16, 32, 32
    env = make_env(host_scenes(N, M, E), N, M, omega)
    got = launch(env, 16, 0)
    single = env.search_assignments(None)
    torch.cuda.synchronize()
    J, Js = got[1].cpu().numpy(), single[1].cpu().numpy()
    print(f"omega {omega}: {int((J > Js).sum())} of {E} rows above the single search, mean J {Js.mean():.5f} -> "
          f"{J.mean():.5f}")
    assert bool((J >= Js).all()) and int((J > Js).sum()) >= 8
    check_choice(f"headline omega {omega}", got)
    other = launch(env, 16, 1)
    assert torch.equal(other[4][:, 0], got[4][:, 0]) and not torch.equal(other[4], got[4])  # another seed, other starts
    assert bool((other[1] >= single[1]).all())


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape", [(16, 32, 32), (5, 7, 33)])
def test_under_constraints(shape, omega):
    """random_constraints' arrays, R = 5, from the fixed ids alone and with them written into random
    ids: the restatement as above and the guarantees on the output; some random start is cut down."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    for name, base in (("the fixed ids", None), ("random ids", random_starts(N, M, E))):
        start, fixed = with_fixed(base, fixed_ids)
        got = run_and_compare(f"{shape} omega {omega} constrained from {name}", env, omega, 5, 2, start, allowed, fixed,
                              capacity)
        single = env.search_assignments_constrained(dev(env, start), dev(env, allowed), dev(env, fixed),
                                                    dev(env, capacity))
        torch.cuda.synchronize()
        assert bool((got[1] >= single[1]).all())
    run_and_compare(f"{shape} omega {omega} capacity alone", env, omega, 5, 2, None, None, None, capacity)


@pytest.mark.parametrize("omega", OMEGAS)
def test_never_above_the_optimum(omega):
    """(16, 32, 8): J <= exact_assignments' J + the bar in every row, unconstrained and constrained."""
    N, M, E = 16, 32, 8
    env = make_env(host_scenes(N, M, E), N, M, omega)
    allowed, capacity, fixed_ids = random_constraints(N, M, E)
    start, fixed = with_fixed(None, fixed_ids)
    for con in ((None, None, None, None), (start, allowed, fixed, capacity)):
        got = launch(env, 16, 0, *con)
        best = env.exact_assignments(*(dev(env, x) for x in con))
        torch.cuda.synchronize()
        J, Jx = got[1].cpu().numpy(), best[1].cpu().numpy()
        print(f"omega {omega}, constraints {con[1] is not None}: share of the optimum {J.mean() / Jx.mean():.5f}, "
              f"{int((J >= Jx - bar(Jx)).sum())} of {E} rows optimal")
        assert bool((J <= Jx + bar(Jx)).all()), (J, Jx)
        assert bool((got[4].cpu().numpy() <= Jx[:, None] + bar(Jx)[:, None]).all())


def test_determinism_stride_rows_in_place_and_read_only():
    N, M, E, omega, K = 5, 7, 33, 0.5, 3
    dec = decoded_env(host_scenes(N, M, E), N, M, omega, K)
    names = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")
    before = {k: getattr(dec, k).clone() for k in names}
    before.update({"scene/" + k: t.clone() for k, t in dec._scene.items()})
    best, _, _, asg = dec.select_best(K)
    assert bool((best >= 0).all())
    allowed, capacity, fixed_ids = random_constraints(N, M, E)  # indexed by row, not by env
    start, fixed = with_fixed(asg.cpu().numpy(), fixed_ids)
    first = run_and_compare("from best-of-3, stride 3", dec, omega, 5, 9, start, allowed, fixed, capacity, stride=K, rows=E)
    again = launch(dec, 5, 9, start, allowed, fixed, capacity, stride=K, rows=E)
    for x, y in zip(first, again):
        assert torch.equal(x, y)                      # the same seed: bitwise the same
    other = launch(dec, 5, 10, start, allowed, fixed, capacity, stride=K, rows=E)
    assert torch.equal(other[4][:, 0], first[4][:, 0])   # replica 0 does not look at the seed
    run_and_compare("from best-of-3, stride 3, 7 rows", dec, omega, 5, 9, start[:7].copy(), allowed[:7].copy(),
                    fixed[:7].copy(), capacity[:7].copy(), stride=K, rows=7)
    bad = start.copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = 2 ** 31 - 1, -2 ** 31, M + 5
    run_and_compare("invalid ids", dec, omega, 5, 9, bad, stride=K, rows=E)
    con = [dev(dec, x) for x in (allowed, fixed, capacity)]
    kept = [x.clone() for x in con]
    buf = dev(dec, start)
    b = dec.search_assignments_multistart(buf, *con, restarts=5, seed=9, stride=K, rows=E, out=buf)
    torch.cuda.synchronize()
    assert b[0].data_ptr() == buf.data_ptr()
    for x, y in tuple(zip(b, first[:4])) + tuple(zip(con, kept)):
        assert torch.equal(x, y)
    ws = dec._multistart_ws
    dec.search_assignments_multistart(None, restarts=2, stride=K, rows=E)
    assert dec._multistart_ws is ws                   # the workspace is kept while it is large enough
    for k in names:
        assert torch.equal(getattr(dec, k), before[k]), k
    for k, t in dec._scene.items():
        assert torch.equal(t, before["scene/" + k]), k


def _fields(r):
    return (r.assignment, r.J, r.covered, r.best_replica, r.steps, r.replica_J, r.decoded_J, r.refine_stats)


def test_through_the_solver():
    """solve(restarts=4) is the stand-alone call on the decode's assignment with the call's seed;
    restarts = 0 is today's solve bitwise; baseline(restarts=4) is never below baseline(exchanges=32);
    with constraints the call with the fixed ids written in."""
    from uavhip import AllocationSolver, Constraints
    N, M, S, K = 16, 32, 8, 2
    solver = AllocationSolver(gpu_policy(N, M, 1), N, M, samples=K)
    r0 = solver.solve(num_scenes=S, seed=5)
    for kw in (dict(), dict(refine=32), dict(refine=32, exchanges=32)):
        for x, y in zip(_fields(solver.solve(num_scenes=S, seed=5, **kw)),
                        _fields(solver.solve(num_scenes=S, seed=5, restarts=0, **kw))):
            assert (x is None and y is None) or torch.equal(x, y)
    today = solver.solve(num_scenes=S, seed=5, refine=32, exchanges=32)
    rx = solver.solve(num_scenes=S, seed=5, refine=32, exchanges=32, restarts=4)
    env = solver.env
    alone = env.search_assignments_multistart(r0.assignment, restarts=4, seed=5, stride=K, rows=S)
    torch.cuda.synchronize()
    for x, y in zip((rx.assignment, rx.J, rx.covered, rx.refine_stats), alone):
        assert torch.equal(x, y)
    assert rx.refine_stats.shape == (S, 10) and torch.equal(rx.decoded_J, r0.J) and bool((rx.J >= today.J).all())
    for x, y in zip(_fields(rx)[3:6], _fields(r0)[3:6]):
        assert torch.equal(x, y)
    assert rx.cpu().refine_stats.shape == (S, 10)
    bx = solver.baseline(num_scenes=S, seed=5, exchanges=32)
    bm = solver.baseline(num_scenes=S, seed=5, exchanges=32, restarts=4)
    alone = solver.env.search_assignments_multistart(None, restarts=4, seed=5, stride=K, rows=S)
    torch.cuda.synchronize()
    for x, y in zip((bm.assignment, bm.J, bm.covered, bm.refine_stats), alone):
        assert torch.equal(x, y)
    assert bm.decoded_J is None and bool((bm.J >= bx.J).all())
    for x, y in zip(_fields(bx)[:6] + (bx.refine_stats,),
                    _fields(solver.baseline(num_scenes=S, seed=5, exchanges=32, restarts=0))[:6] + (bx.refine_stats,)):
        assert torch.equal(x, y)
    print(f"16 x 32, {S} scenes: mean J polished {today.J.mean().item():.4f} -> {rx.J.mean().item():.4f} with 4 "
          f"restarts; baseline {bx.J.mean().item():.4f} -> {bm.J.mean().item():.4f}")
    allowed, capacity, fixed_ids = random_constraints(N, M, S)
    con = Constraints(allowed=torch.from_numpy(allowed), capacity=capacity, fixed_ids=torch.from_numpy(fixed_ids))
    rc = solver.solve(num_scenes=S, seed=5, refine=32, exchanges=32, constraints=con, restarts=4)
    env = solver.env
    start, fixed = with_fixed(r0.assignment.cpu().numpy(), fixed_ids)
    alone = env.search_assignments_multistart(dev(env, start), dev(env, allowed), dev(env, fixed), dev(env, capacity),
                                              restarts=4, seed=5, stride=K, rows=S)
    torch.cuda.synchronize()
    for x, y in zip((rc.assignment, rc.J, rc.covered, rc.refine_stats), alone):
        assert torch.equal(x, y)
    check_guarantees("solve, constraints, restarts", rc.assignment.cpu().numpy(), tables(env, K, S)[4], start, allowed,
                     fixed, capacity)
    single = solver.solve(num_scenes=S, seed=5, refine=32, exchanges=32, constraints=con)
    assert bool((rc.J >= single.J).all())


# what `--refine 32 --baseline --exchanges 32` printed before --restarts existed, in its order
PARENT_KEYS = ["scenes", "samples", "N", "M", "seed", "mean_J", "best_J", "mean_covered", "mean_steps", "unfinished",
               "scenes_per_s", "mean_J_decoded", "mean_J_refined", "mean_exchanges", "mean_J_baseline",
               "policy_beats_baseline", "mean_J_baseline_exchange"]


def test_command_line_keys(tmp_path, capsys):
    """--restarts 4 adds mean_J_multistart (with --optimum also the two shares); without the flag the key
    list is the one from before the flag."""
    import copy

    from uavhip import solve
    N, M = 16, 32
    ck = tmp_path / "policy.pth"
    torch.save(copy.deepcopy(gpu_policy(N, M, 1)).cpu().state_dict(), ck)
    argv = ["--checkpoint", str(ck), "--scenes", "8", "--samples", "2", "--uavs", str(N), "--targets", str(M),
            "--refine", "32", "--baseline", "--exchanges", "32"]
    solve.main(argv)
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert list(plain) == PARENT_KEYS
    solve.main(argv + ["--restarts", "4"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert list(out) == PARENT_KEYS + ["mean_J_multistart"]
    assert all(out[k] == plain[k] for k in plain if k != "scenes_per_s")
    assert out["mean_J_multistart"] >= out["mean_J_baseline_exchange"]
    solve.main(argv + ["--restarts", "4", "--optimum"])
    opt = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert [k for k in opt if "multistart" in k] == ["mean_J_multistart", "multistart_over_optimal", "multistart_is_optimal"]
    assert opt["mean_J_multistart"] == out["mean_J_multistart"]
    assert opt["baseline_exchange_over_optimal"] <= opt["multistart_over_optimal"] <= 1.0 + RTOL_J
    assert opt["baseline_exchange_is_optimal"] <= opt["multistart_is_optimal"] <= 1.0
