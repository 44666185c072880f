"""uavhip_search_assignments on the GPU (k_search): the kernel against search_np, the Python restatement
of the exchange-move rule (tests/test_search_host.py), fed the pair tables read back from the device
-- assignments, all six stats and covered exactly, J to the project's reward bar -- and the layers
above it: VecUAVEnv.search_assignments, AllocationSolver.solve(refine=, exchanges=) / baseline and
ImitationRun(teacher_exchanges=).

Shapes (N, M, E): the register-column path at its three capacities (4 x 4 and 5 x 7: 8; 16 x 32: 16;
none of the project's cases has 16 < N <= 32 with M <= 64, so 17 x 20 is added for the third), the
streamed path (33 x 34) and two targets per lane (12 x 70, 34 x 66, 8 x 128); every E leaves the last
workgroup of four waves partial or is a multiple of it (32)."""
import json
import os

import numpy as np
import pytest
import torch

import capi_host
from test_gpu_refine import decoded_env, make_env, tables
from test_gpu_solve import gpu_policy
from test_refine_host import OMEGAS, RTOL_J, host_scenes, random_starts
from test_search_host import CAPS, NOTHING_TO_DO, SHAPES, check_search_conditions, search_rows

pytestmark = pytest.mark.gpu

# want_exchange of check_search_conditions per shape: the host test's cases exchange, 4 x 4 has nothing to
# do, the two added shapes may do either
CASES = [(s, True) for s in SHAPES] + [(NOTHING_TO_DO, False), ((8, 128, 3), None), ((17, 20, 5), None)]


_entry_point = capi_host._entry_point("uavhip_search_assignments")


def run_and_compare(label, env, omega, start, stride=1, rows=None, max_exchanges=CAPS[0], max_sweeps=CAPS[1], **kw):
    """One launch against search_np on the device's tables. Returns (the restatement's rows, the launch's outputs)."""
    got = env.search_assignments(None if start is None else torch.from_numpy(start).to(env.device), stride=stride,
                                 rows=rows, max_exchanges=max_exchanges, max_sweeps=max_sweeps, **kw)
    torch.cuda.synchronize()
    asg, J, cov, st = (t.cpu().numpy() for t in got)
    want = search_rows(*tables(env, stride, rows), omega, start, max_exchanges, max_sweeps)
    err = np.abs(J - want[1]) / np.maximum(1.0, np.abs(want[1]))
    print(f"{label}: {len(J)} rows, sweeps {want[3][:, 0].min()}..{want[3][:, 0].max()}, exchanges "
          f"{want[3][:, 4].min()}..{want[3][:, 4].max()}, mean J {want[1].mean():.6f}, max J err {err.max():.2e} "
          f"(bar {RTOL_J:g})")
    assert asg.dtype == np.int32 and np.array_equal(asg, want[0]), label
    assert st.shape == (len(J), 6) and np.array_equal(st, want[3]), label
    assert np.array_equal(cov, want[2]), label
    assert bool((err <= RTOL_J).all()), (label, float(err.max()))
    return want, got


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("shape,want_exchange", CASES)
def test_kernel_is_the_restatement(shape, want_exchange, omega):
    """Against search_np; max_exchanges = 0 is refine_assignments bitwise; and J is never below the plain
    refinement's beyond the reward bar (the first phase is that refinement, each exchange has d > 0)."""
    N, M, E = shape
    env = make_env(host_scenes(N, M, E), N, M, omega)
    tag = f"({N}, {M}, {E}) omega {omega}"
    runs = []
    for name, start in (("empty", None), ("random ids", random_starts(N, M, E))):
        want, got = run_and_compare(f"{tag} from {name}", env, omega, start)
        runs.append(want)
        dev_start = None if start is None else torch.from_numpy(start).to(env.device)
        plain = env.refine_assignments(dev_start)
        zero = env.search_assignments(dev_start, max_exchanges=0)
        torch.cuda.synchronize()
        for x, y in zip(zero[:3], plain[:3]):
            assert torch.equal(x, y), tag
        assert torch.equal(zero[3][:, :4], plain[3]) and not bool(zero[3][:, 4:].any()), tag
        J, Jr = got[1], plain[1]
        gain = (J - Jr).cpu().numpy()
        print(f"{tag} from {name}: J - J_refine in [{gain.min():.3e}, {gain.max():.3e}], mean {gain.mean():.4f}")
        assert bool((J >= Jr - RTOL_J * Jr.abs().clamp(min=1.0)).all()), tag
    check_search_conditions(tag, runs, want_exchange=want_exchange, want_two=(N, M) == (16, 32))


def test_cap_and_continuation():
    """max_exchanges = 1 at 16 x 32 stops the rows that need more with scan_clean = 0; feeding its
    output back with a cap of 31 ends on the one-call result, assignments and J bitwise."""
    N, M, E, omega = 16, 32, 32, 0.0
    env = make_env(host_scenes(N, M, E), N, M, omega)
    full, got = run_and_compare("cap 32", env, omega, None)
    need = full[3][:, 4]
    assert need.max() >= 2 and need.min() <= 1, need
    one, first = run_and_compare("cap 1", env, omega, None, max_exchanges=1)
    assert np.array_equal(one[3][:, 4], np.minimum(need, 1))
    assert np.array_equal(one[3][:, 5], (need <= 1).astype(np.int32))
    assert bool((one[3][:, 2] == 1).all())
    second = env.search_assignments(first[0], max_exchanges=31)
    torch.cuda.synchronize()
    assert torch.equal(second[0], got[0]) and torch.equal(second[1], got[1]) and torch.equal(second[2], got[2])
    st = second[3].cpu().numpy()
    assert np.array_equal(st[:, 4], need - np.minimum(need, 1)) and bool((st[:, 5] == 1).all())
    # no sweeps: the scan alone, an exchange, no sweep after it
    run_and_compare("cap 3, no sweeps", env, omega, random_starts(N, M, E), max_exchanges=3, max_sweeps=0)


def test_stride_rows_invalid_ids_in_place_and_read_only():
    N, M, E, omega, K = 5, 7, 33, 0.5, 3
    dec = decoded_env(host_scenes(N, M, E), N, M, omega, K)
    names = ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window")
    before = {k: getattr(dec, k).clone() for k in names}
    before.update({"scene/" + k: t.clone() for k, t in dec._scene.items()})
    best, _, _, asg = dec.select_best(K)
    assert bool((best >= 0).all())
    start = asg.cpu().numpy()
    run_and_compare("from best-of-3, stride 3", dec, omega, start, stride=K, rows=E)
    run_and_compare("from best-of-3, stride 3, 7 rows", dec, omega, start[:7].copy(), stride=K, rows=7)
    bad = start.copy()
    sel = np.random.default_rng(2).random((E, N))
    bad[sel < 0.1] = M + 5
    bad[(sel >= 0.1) & (sel < 0.2)] = -3
    bad[0, 0], bad[1, 1] = 2 ** 31 - 1, -2 ** 31
    want, _ = run_and_compare("invalid ids", dec, omega, bad, stride=K, rows=E)
    assert want[3][:, 3].sum() >= (sel < 0.2).sum() > 0
    buf = torch.from_numpy(bad).to(dec.device)
    a, J, cov, st = dec.search_assignments(buf.clone(), stride=K, rows=E)
    b, J2, cov2, st2 = dec.search_assignments(buf, stride=K, rows=E, out=buf)
    torch.cuda.synchronize()
    assert b.data_ptr() == buf.data_ptr()
    for x, y in ((a, b), (J, J2), (cov, cov2), (st, st2)):
        assert torch.equal(x, y)
    for k in names:
        assert torch.equal(getattr(dec, k), before[k]), k
    for k, t in dec._scene.items():
        assert torch.equal(t, before["scene/" + k]), k


def _fields(r):
    return (r.assignment, r.J, r.covered, r.best_replica, r.steps, r.replica_J, r.decoded_J, r.refine_stats)


def test_through_the_solver():
    from uavhip import AllocationSolver
    N, M, S, K = 16, 32, 8, 2
    solver = AllocationSolver(gpu_policy(N, M, 1), N, M, samples=K)
    r0 = solver.solve(num_scenes=S, seed=5)
    today = solver.solve(num_scenes=S, seed=5, refine=32)
    same = solver.solve(num_scenes=S, seed=5, refine=32, exchanges=0)
    for x, y in zip(_fields(today), _fields(same)):
        assert torch.equal(x, y)
    assert today.refine_stats.shape == (S, 4)
    rx = solver.solve(num_scenes=S, seed=5, refine=32, exchanges=32)
    alone = solver.env.search_assignments(r0.assignment, stride=K, rows=S, max_exchanges=32, max_sweeps=32)
    torch.cuda.synchronize()
    for x, y in zip((rx.assignment, rx.J, rx.covered, rx.refine_stats), alone):
        assert torch.equal(x, y)
    assert rx.refine_stats.shape == (S, 6) and torch.equal(rx.decoded_J, r0.J)
    for x, y in zip(_fields(rx)[3:6], _fields(r0)[3:6]):
        assert torch.equal(x, y)
    assert bool((rx.J >= today.J - RTOL_J * today.J.abs().clamp(min=1.0)).all())
    print(f"solve 16 x 32, {S} scenes, K = {K}: mean J refined {today.J.mean().item():.4f}, with exchanges "
          f"{rx.J.mean().item():.4f}, exchanges {rx.refine_stats[:, 4].tolist()}")
    assert rx.cpu().refine_stats.shape == (S, 6)
    b0 = solver.baseline(num_scenes=S, seed=5)
    b0x = solver.baseline(num_scenes=S, seed=5, exchanges=0)
    for x, y in zip(_fields(b0)[:6] + (b0.refine_stats,), _fields(b0x)[:6] + (b0x.refine_stats,)):
        assert torch.equal(x, y)
    bx = solver.baseline(num_scenes=S, seed=5, exchanges=32)
    alone = solver.env.search_assignments(None, stride=K, rows=S)
    torch.cuda.synchronize()
    for x, y in zip((bx.assignment, bx.J, bx.covered, bx.refine_stats), alone):
        assert torch.equal(x, y)
    assert bx.decoded_J is None and bool((bx.J >= b0.J - RTOL_J * b0.J.abs().clamp(min=1.0)).all())
    print(f"baseline: mean J {b0.J.mean().item():.4f}, with exchanges {bx.J.mean().item():.4f}")


def test_command_line_keys(tmp_path, capsys):
    """--exchanges: mean_exchanges with --refine; with --baseline the plain mean_J_baseline stays what it
    is without the flag and mean_J_baseline_exchange stands beside it; without the flag no key changes."""
    import copy

    from uavhip import solve
    N, M = 16, 32
    ck = tmp_path / "policy.pth"
    torch.save(copy.deepcopy(gpu_policy(N, M, 1)).cpu().state_dict(), ck)
    argv = ["--checkpoint", str(ck), "--scenes", "8", "--samples", "2", "--uavs", str(N), "--targets", str(M)]
    solve.main(argv + ["--refine", "32", "--baseline"])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "mean_exchanges" not in plain and "mean_J_baseline_exchange" not in plain
    solve.main(argv + ["--refine", "32", "--baseline", "--exchanges", "32"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    keys = [k for k in out if k not in ("mean_exchanges", "mean_J_baseline_exchange")]
    assert keys == list(plain) and list(out)[:11] == list(plain)[:11]
    assert out["mean_J_baseline"] == plain["mean_J_baseline"] and out["mean_J_decoded"] == plain["mean_J_decoded"]
    assert out["mean_exchanges"] > 0
    assert out["mean_J_refined"] >= plain["mean_J_refined"] - RTOL_J * abs(plain["mean_J_refined"])
    assert out["mean_J_baseline_exchange"] >= out["mean_J_baseline"] - RTOL_J * abs(out["mean_J_baseline"])
    solve.main(argv + ["--baseline", "--exchanges", "32"])  # without --refine the flag is the baseline's alone
    base = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "mean_exchanges" not in base and "mean_J_refined" not in base
    assert base["mean_J_baseline_exchange"] == out["mean_J_baseline_exchange"]
    with pytest.raises(SystemExit):
        solve.main(argv + ["--exchanges", "-1"])


def test_through_imitation(tmp_path):
    from uavhip.imitate import ImitationRun
    run = ImitationRun(64, 4, 4, 64, str(tmp_path / "x"), seed=3, epochs=1, teacher_exchanges=4)
    out = run.fit(1)
    lines = [json.loads(x) for x in open(tmp_path / "x" / "progress.jsonl")]
    assert [x["iteration"] for x in lines] == [1] and lines[0]["rows"] > 0
    assert np.isfinite(lines[0]["teacher_mean_J"]) and np.isfinite(lines[0]["nll_after"])
    assert os.path.exists(out["final_model"])
    # the teacher's J is the search's on the run's own scenes
    _, J, _, st = run.env.search_assignments(None, max_exchanges=4, max_sweeps=32)
    assert abs(float(J.mean()) - lines[0]["teacher_mean_J"]) <= RTOL_J * max(1.0, abs(float(J.mean())))
