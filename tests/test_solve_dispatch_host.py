"""Which search AllocationSolver launches for which options, on the host (no GPU, no library call): the
solver runs on a recording stand-in for its env -- the solver wrappers' names and signatures, host tensors
of their shapes back, every call logged -- so a slip in the ladder of solve() / baseline() / optimum()
shows without a device. What the wrappers themselves check and launch is the other host and GPU tests'."""
import contextlib

import pytest
import torch

from test_exact_host import _OnGpu

S, K, N, M = 3, 2, 4, 5
U64 = 2 ** 64 - 1
DECODED_J = [1.0, 2.0, 3.0]


class _Env:
    """The env of S * K replicas as the solver sees it after _scene_env: the attributes the wrappers read
    and the seven wrappers, each logging (short name, its arguments by name) and returning fresh host
    tensors; call c of a test returns J = 100 c in every row."""

    def __init__(self):
        self.E, self.N, self.M, self.device = S * K, N, M, torch.device("cpu")
        self.log = []

    def _call(self, name, kw, last):
        del kw["self"]
        self.log.append((name, kw))
        rows = kw["rows"]
        return (torch.full((rows, N), len(self.log), dtype=torch.int32),
                torch.full((rows,), 100.0 * len(self.log), dtype=torch.float64),
                torch.ones(rows, dtype=torch.int32), torch.zeros((rows,) + last, dtype=torch.int32))

    def assigned_target_ids(self):
        return torch.arange(self.E * N).view(self.E, N) % M

    def refine_assignments(self, assignment=None, stride=1, rows=None, max_sweeps=32, out=None, J=None, covered=None,
                           stats=None):
        return self._call("refine", dict(locals()), (4,))

    def search_assignments(self, assignment=None, stride=1, rows=None, max_exchanges=32, max_sweeps=32, out=None,
                           J=None, covered=None, stats=None):
        return self._call("search", dict(locals()), (6,))

    def search_assignments_constrained(self, assignment=None, allowed=None, fixed=None, capacity=None, stride=1,
                                       rows=None, max_exchanges=32, max_sweeps=32, out=None, J=None, covered=None,
                                       stats=None):
        return self._call("constrained", dict(locals()), (8,))

    def search_assignments_multistart(self, assignment=None, allowed=None, fixed=None, capacity=None, restarts=16,
                                      seed=0, stride=1, rows=None, max_exchanges=32, max_sweeps=32, out=None, J=None,
                                      covered=None, stats=None, J_all=None, starts=None):
        return self._call("multistart", dict(locals()), (10,))

    def exact_assignments(self, assignment=None, allowed=None, fixed=None, capacity=None, stride=1, rows=None, out=None,
                          J=None, covered=None, stats=None, max_workspace_bytes=1 << 30):
        return self._call("exact", dict(locals()), (2,))

    def exact_free_assignments(self, assignment=None, *, max_free, allowed=None, fixed=None, capacity=None, stride=1,
                               rows=None, out=None, J=None, covered=None, stats=None, max_workspace_bytes=None):
        return self._call("exact_free", dict(locals()), (4,))

    def lns_assignments(self, assignment, *, rounds, free, mode="targets", seed=0, allowed=None, fixed=None,
                        capacity=None, stride=1, rows=None):
        return self._call("lns", dict(locals()), ())  # the fourth is `improved` [rows]


def _stub_decode(monkeypatch, solver_cls):
    """solve()'s decode replaced: what select_best would leave, DECODED_J and the assignment of all 7s."""
    from uavhip.solve import Allocation

    def decode(self, env, S_, seed, max_steps, trace):
        zi = torch.zeros(S_, dtype=torch.int32)
        return Allocation(torch.full((S_, N), 7, dtype=torch.int32), torch.tensor(DECODED_J, dtype=torch.float64),
                          zi + 2, zi.clone(), zi + 9, torch.zeros(S_, K, dtype=torch.float64))
    monkeypatch.setattr(solver_cls, "_decode", decode)


@pytest.fixture
def solver(monkeypatch):
    from uavhip import AllocationSolver
    s = AllocationSolver(_OnGpu(), N, M, samples=K)
    s.device = torch.device("cpu")  # where Constraints.on puts its tensors
    env = _Env()
    monkeypatch.setattr(AllocationSolver, "_scene_env", lambda self, scenes, S_, seed: env)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    _stub_decode(monkeypatch, AllocationSolver)
    return s, env


def _constraints():
    from uavhip import Constraints
    fixed_ids = torch.full((S, N), -2, dtype=torch.int32)
    fixed_ids[0, 1], fixed_ids[2, 3] = 4, -1
    return Constraints(allowed=torch.ones(S, N, M, dtype=torch.bool), capacity=torch.full((S, M), 2, dtype=torch.int32),
                       fixed_ids=fixed_ids)


def _laid_over(fixed_ids, start):
    return torch.where(fixed_ids != -2, fixed_ids, start)


def _names(env):
    return [name for name, _ in env.log]


# options -> the wrappers launched, in order, for baseline(...) and for solve(refine=4, ...)
RUNGS = [({}, ["refine"]),
         (dict(exchanges=2), ["search"]),
         (dict(constraints=True), ["constrained"]),
         (dict(exchanges=2, constraints=True), ["constrained"]),
         (dict(restarts=3), ["multistart"]),
         (dict(restarts=3, constraints=True, lns_rounds=2), ["multistart", "lns"]),
         (dict(lns_rounds=1), ["refine", "lns"])]


def _options(opts):
    opts = dict(opts)
    if opts.get("constraints"):
        opts["constraints"] = _constraints()
    return opts


def _check_rows_and_caps(env, opts, sweeps, seed):
    for name, kw in env.log:
        assert kw["stride"] == K and kw["rows"] == S, (name, kw)
        if name in ("refine", "search", "constrained", "multistart"):
            assert kw["max_sweeps"] == sweeps
        if name in ("search", "constrained", "multistart"):
            assert kw["max_exchanges"] == opts.get("exchanges", 0)
        if name == "multistart":
            assert kw["restarts"] == opts["restarts"] and kw["seed"] == seed & U64
        if name == "lns":
            assert kw["rounds"] == opts["lns_rounds"] and kw["free"] == 12 and kw["mode"] == "targets"
            assert kw["seed"] == seed & U64
        if name in ("refine", "search"):
            assert "fixed" not in kw and "allowed" not in kw
        elif opts.get("constraints"):
            c = opts["constraints"]
            assert torch.equal(kw["allowed"], c.allowed.to(torch.uint8)) and torch.equal(kw["capacity"], c.capacity)
            assert torch.equal(kw["fixed"], (c.fixed_ids != -2).to(torch.uint8))
        else:
            assert kw["allowed"] is None and kw["capacity"] is None and kw["fixed"] is None


@pytest.mark.parametrize("opts, want", RUNGS)
@pytest.mark.parametrize("seed", [7, -1])
def test_baseline_dispatch(solver, opts, want, seed):
    s, env = solver
    opts = _options(opts)
    b = s.baseline(num_scenes=S, seed=seed, max_sweeps=5, **opts)
    assert _names(env) == want
    _check_rows_and_caps(env, opts, 5, seed)
    start = env.log[0][1]["assignment"]
    if opts.get("constraints"):  # the committed UAVs' ids and nothing else
        assert torch.equal(start, _laid_over(opts["constraints"].fixed_ids, torch.full((S, N), -1, dtype=torch.int32)))
    else:
        assert start is None
    assert b.refine_stats.shape == (S, {"refine": 4, "search": 6, "constrained": 8, "multistart": 10}[want[0]])
    assert (b.lns_J_before is not None) == ("lns" in want)
    if "lns" in want:
        assert b.lns_J_before.tolist() == [100.0] * S and b.J.tolist() == [200.0] * S
        assert torch.equal(env.log[1][1]["assignment"], torch.full((S, N), 1, dtype=torch.int32))  # the search's result
    else:
        assert b.J.tolist() == [100.0] * S
    assert b.decoded_J is None and b.best_replica.tolist() == [0] * S and b.replica_J.shape == (S, K)


def test_optimum_dispatch(solver):
    s, env = solver
    c = _constraints()
    o = s.optimum(num_scenes=S, seed=7, constraints=c, max_workspace_bytes=12345)
    assert _names(env) == ["exact"]
    kw = env.log[0][1]
    assert kw["stride"] == K and kw["rows"] == S and kw["max_workspace_bytes"] == 12345
    assert torch.equal(kw["assignment"], _laid_over(c.fixed_ids, torch.full((S, N), -1, dtype=torch.int32)))
    assert torch.equal(kw["fixed"], (c.fixed_ids != -2).to(torch.uint8)) and torch.equal(kw["capacity"], c.capacity)
    assert o.refine_stats.shape == (S, 2) and o.lns_J_before is None and o.J.tolist() == [100.0] * S
    env.log.clear()
    s.optimum(num_scenes=S)
    assert _names(env) == ["exact"]
    kw = env.log[0][1]
    assert kw["assignment"] is None and kw["allowed"] is None and kw["fixed"] is None and kw["capacity"] is None


@pytest.mark.parametrize("opts, want", RUNGS)
@pytest.mark.parametrize("seed", [7, -1])
def test_solve_dispatch(solver, opts, want, seed):
    s, env = solver
    opts = _options(opts)
    r = s.solve(num_scenes=S, seed=seed, refine=4, **opts)
    assert _names(env) == want
    _check_rows_and_caps(env, opts, 4, seed)
    start = env.log[0][1]["assignment"]
    decoded = torch.full((S, N), 7, dtype=torch.int32)
    if opts.get("constraints"):  # the fixed ids laid over the decoded assignment
        assert torch.equal(start, _laid_over(opts["constraints"].fixed_ids, decoded))
    else:
        assert torch.equal(start, decoded)
    assert r.decoded_J.tolist() == DECODED_J  # the decode's J, not the search's
    assert r.J.tolist() == [100.0 * len(want)] * S
    assert r.refine_stats.shape == (S, {"refine": 4, "search": 6, "constrained": 8, "multistart": 10}[want[0]])
    assert (r.lns_J_before is not None) == ("lns" in want)
    assert r.steps.tolist() == [9] * S and r.start_J is None  # the decode-only fields are the decode's


def test_solve_without_refine_launches_no_search(solver):
    s, env = solver
    r = s.solve(num_scenes=S, seed=7)
    assert env.log == [] and r.J.tolist() == DECODED_J and r.decoded_J is None and r.refine_stats is None
    r = s.solve(num_scenes=S, seed=7, lns_rounds=1, lns_free=3, lns_mode="random")
    assert _names(env) == ["lns"]
    kw = env.log[0][1]
    assert (kw["rounds"], kw["free"], kw["mode"], kw["seed"], kw["stride"], kw["rows"]) == (1, 3, "random", 7, K, S)
    assert torch.equal(kw["assignment"], torch.full((S, N), 7, dtype=torch.int32)) and kw["fixed"] is None
    assert r.lns_J_before.tolist() == DECODED_J and r.J.tolist() == [100.0] * S and r.decoded_J is None


@pytest.mark.parametrize("constrained", [False, True])
def test_solve_from_replicas(solver, constrained):
    s, env = solver
    c = _constraints() if constrained else None
    r = s.solve(num_scenes=S, seed=-1, refine=4, exchanges=2, restarts=2, starts="replicas", constraints=c)
    assert _names(env) == ["multistart"]
    kw = env.log[0][1]
    assert kw["assignment"] is None and kw["starts"].shape == (S, K, N) and kw["starts"].dtype == torch.int32
    assert kw["starts"].is_contiguous() and kw["J_all"].shape == (S, 2) and r.start_J is kw["J_all"]
    assert (kw["restarts"], kw["seed"], kw["stride"], kw["rows"], kw["max_exchanges"], kw["max_sweeps"]) == \
        (2, U64, K, S, 2, 4)
    given = env.assigned_target_ids().to(torch.int32).view(S, K, N)
    if constrained:  # the fixed ids over every one of the K starts
        ids = c.fixed_ids.view(S, 1, N)
        assert torch.equal(kw["starts"], _laid_over(ids, given))
        assert torch.equal(kw["fixed"], (c.fixed_ids != -2).to(torch.uint8))
    else:
        assert torch.equal(kw["starts"], given) and kw["fixed"] is None
    assert r.decoded_J.tolist() == DECODED_J and r.refine_stats.shape == (S, 10)
