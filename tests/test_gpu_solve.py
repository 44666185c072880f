"""Batched allocation inference on the GPU: uavhip_decode_steps (actor-only decode to each env's
episode end), uavhip_select_best and AllocationSolver, against the CPU oracle env, the torch fp32
policy and the training rollout's actor.

The test policy. A freshly initialised policy decodes "skip" at every step (the last actor layer has
gain 0.01 and a logit gap of constant sign), which would make every check below vacuous. So the policy
is built on the CPU, deterministically: torch.manual_seed(s); the last actor layer's weight <-
randn(2, 64) from a seeded generator; its bias[1] -= the median logit gap over the states of a few
random-action oracle episodes (p(assign) = 0.3). Decoding then mixes both actions and the episodes
of one batch end at different steps."""
import copy
import functools
import random

import numpy as np
import pytest
import torch

from conftest import cases, sub
from test_solve_host import select_best_np

pytestmark = pytest.mark.gpu

MARGIN = 1e-3      # |l1 - l0| below which a greedy action is not compared with the torch policy: 100 x
                   # the 1e-5 at which test_fused_policy_vs_reference compares logits (here O(1 - 10))
MAX_SKIPPED = 0.02  # share of steps allowed inside the margin (a condition of the case, not a tolerance)
RTOL_J = 1e-12     # the project's reward bar against the oracle

# (N, M, E): grouped env path with one partial workgroup; E odd (one env per wave, three workgroups,
# an unpaired last env); grouped path, two full workgroups at the workload's N, M; N, M > 32 (the
# wave path with lanes beyond 32, up to 1122 steps: the ring wraps many times)
SHAPES = [(4, 4, 6), (5, 7, 33), (16, 32, 32), (33, 34, 3)]


def _prm():
    from uavhip.config import cfg, params_vector
    return params_vector(cfg)


@functools.lru_cache(maxsize=None)
def host_scenes(N, M, n, seed):
    from uavhip.config import Config
    from uavhip.scene import generate_scene
    c = Config()
    c.NUM_UAVS, c.NUM_TARGETS = N, M
    np.random.seed(seed)
    random.seed(seed)
    return tuple(generate_scene(c) for _ in range(n))


@functools.lru_cache(maxsize=None)
def cpu_policy(N, M, seed):
    """The test policy for N x M scenes (module docstring), on the CPU."""
    import oracle
    from uavhip.policy import TransformerActorCritic
    torch.manual_seed(seed)
    net = TransformerActorCritic()
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    wins = []
    for s in host_scenes(N, M, 3, 1000 + seed):
        ref = oracle.OracleEnv(s, _prm())
        obs, done = ref.reset(), False
        while not done:
            wins.append(obs)
            obs, _, done, _ = ref.step(int(rng.random() < 0.3))
    with torch.no_grad():
        net.actor_head[2].weight.copy_(torch.randn(2, 64, generator=g))
        logits, _ = net.heads(torch.from_numpy(np.stack(wins)))
        net.actor_head[2].bias[1] -= (logits[:, 1] - logits[:, 0]).median()
    return net


def gpu_policy(N, M, seed):
    return copy.deepcopy(cpu_policy(N, M, seed)).to("cuda")


def make_env(scenes, N, M):
    from uavhip.vec_env import VecUAVEnv
    v = VecUAVEnv(len(scenes), N, M, 1, 1, full_reset_period=0)
    v.load_scenes(list(scenes))
    return v


class Decode:
    """One env set and its decode buffers; run() decodes up to n_max more steps."""

    def __init__(self, net, scenes, N, M):
        from uavhip.policy import rowproj_buffer
        self.net, self.env = net, make_env(scenes, N, M)
        E, dev = self.env.E, self.env.device
        self.E = E
        self.obs2 = torch.zeros(2, E, 5, 14, device=dev)
        self.rp = rowproj_buffer(E, dev)
        self.steps = torch.zeros(E, dtype=torch.int32, device=dev)
        self.fin = torch.full((E,), 9, dtype=torch.uint8, device=dev)
        self.ret = torch.zeros(E, dtype=torch.float64, device=dev)
        self.done_steps = 0
        self.env.reset(episode=1, obs_out=self.obs2[0])

    def run(self, n_max, greedy_stride=1, seed=11, offset=0, stride=0, optional=True):
        """optional=False: without the nullable outputs (action trace, return)."""
        act = torch.full((n_max, self.E), 7, dtype=torch.int8, device=self.env.device) if optional else None
        self.net.decode_steps(self.env, self.obs2, self.rp, self.done_steps, True, self.steps, self.fin, actions=act,
                              ep_return=self.ret if optional else None, n_max=n_max, greedy_stride=greedy_stride,
                              seed=seed, offset=offset, offset_stride=stride)
        torch.cuda.synchronize()
        self.done_steps += n_max
        return act

    def state(self):
        v = self.env
        return [t.clone() for t in (v.istate, v.dstate, v.assigned, v.nh_final, v.nh_pure, v.t_cost, v.n_lock, v.window)]


def oracle_replay(scene, trace, n):
    """Feed trace[:n] to an OracleEnv of `scene`: (windows seen [n, 5, 14], return, final J, covered,
    assigned ids, step at which the episode ended or None)."""
    import oracle
    ref = oracle.OracleEnv(scene, _prm())
    obs, wins, ret, J, cov, end = ref.reset(), [], 0.0, 0.0, 0, None
    for t in range(n):
        assert trace[t] in (0, 1), (t, trace[t])
        assert end is None, f"the trace goes on after the oracle's episode ended at step {end}"
        wins.append(obs)
        obs, r, done, info = ref.step(int(trace[t]))
        ret += r
        J, cov = info[0], int(info[1])
        if done:
            end = t + 1
    return np.stack(wins), ret, J, cov, ref.assigned(), end


def check_against_oracle(d, scenes, N, M, trace):
    """Every env's trace replayed through the oracle: episode end, trace padding, assignment, covered,
    J, return, no error bit. Returns (windows, actions, env index) of all steps."""
    from uavhip import _lib
    steps, fin, ret = d.steps.cpu().numpy(), d.fin.cpu().numpy(), d.ret.cpu().numpy()
    ids = d.env.assigned_target_ids().cpu().numpy()
    ist, dst = d.env.istate.cpu().numpy(), d.env.dstate.cpu().numpy()
    wins, acts, envs = [], [], []
    for e in range(d.E):
        n = int(steps[e])
        assert fin[e] == 1 and N <= n <= N * M, (e, n, fin[e])
        assert (trace[n:, e] == -1).all(), e
        w, r_o, J_o, cov_o, asg_o, end = oracle_replay(scenes[e], trace[:, e], n)
        assert end == n, (e, end, n)
        assert list(ids[e]) == list(asg_o), e
        assert ist[e, _lib.IST["N_COVERED"]] == cov_o, e
        J, r = dst[e, _lib.DST["J"]], ret[e]
        print(f"env {e}: steps {n} J {J:.6f} (oracle {J_o:.6f}, d {abs(J - J_o):.1e}) return {r:.6f} (d {abs(r - r_o):.1e})")
        assert abs(J - J_o) <= RTOL_J * max(1.0, abs(J_o)), (e, J, J_o)
        assert abs(r - r_o) <= RTOL_J * max(1.0, abs(r_o)), (e, r, r_o)
        assert ist[e, _lib.IST["ERROR"]] == 0, e  # later steps of the launch left the finished env alone
        wins.append(w)
        acts.append(trace[:n, e])
        envs.append(np.full(n, e))
    return np.concatenate(wins), np.concatenate(acts), np.concatenate(envs)


@pytest.mark.parametrize("N,M,E", SHAPES)
def test_greedy_decode_replays_through_oracle(N, M, E):
    seed = 1
    scenes = host_scenes(N, M, E, seed)
    d = Decode(gpu_policy(N, M, seed), scenes, N, M)
    trace = d.run(N * M).cpu().numpy()
    wins, acts, _ = check_against_oracle(d, scenes, N, M, trace)
    # the torch fp32 policy on the oracle's windows of all steps, one batched call
    with torch.no_grad():
        logits, _ = cpu_policy(N, M, seed).heads(torch.from_numpy(wins))
    gap = (logits[:, 1] - logits[:, 0]).numpy()
    clear = np.abs(gap) >= MARGIN
    skipped = 1.0 - clear.mean()
    steps = d.steps.cpu().numpy()
    print(f"({N}, {M}, {E}): {len(acts)} steps, assign share {acts.mean():.3f}, episode lengths "
          f"{steps.min()}..{steps.max()}, inside the margin {skipped:.4%}, smallest gap {np.abs(gap).min():.2e}")
    assert skipped <= MAX_SKIPPED
    assert np.array_equal(acts[clear], (gap[clear] > 0).astype(acts.dtype))
    assert 0 < acts.sum() < len(acts), "degenerate case: one action only"
    assert len(set(steps.tolist())) > 1, "degenerate case: every episode has the same length"


@pytest.mark.parametrize("N,M,E", [(16, 32, 32), (5, 7, 33)])
def test_sampled_decode_is_the_rollouts_actor(N, M, E):
    """greedy_stride = 0: the decode samples what uavhip_rollout_steps samples (the same seed, offset
    and stride on identical env copies) -- exactly, the actor path is the same code. Compared over
    the first N steps, before which no env can finish."""
    from uavhip.policy import rowproj_buffer
    seed = 1
    scenes = host_scenes(N, M, E, seed)
    net = gpu_policy(N, M, seed)
    d = Decode(net, scenes, N, M)
    got = d.run(N, greedy_stride=0, seed=5, offset=1000, stride=E + 3)
    env = make_env(scenes, N, M)
    dev = env.device
    obs = torch.zeros(N + 1, E, 5, 14, device=dev)
    env.reset(episode=1, obs_out=obs[0])
    act = torch.zeros(N, E, dtype=torch.int8, device=dev)
    lp, val = torch.zeros(N, E, device=dev), torch.zeros(N, E, device=dev)
    rew = torch.zeros(N, E, dtype=torch.float64, device=dev)
    dn = torch.zeros(N, E, dtype=torch.uint8, device=dev)
    net.rollout_steps(env, obs, rowproj_buffer(E, dev), 0, True, act, lp, val, rew, dn, None, auto_reset=False,
                      seed=5, offset=1000, offset_stride=E + 3)
    torch.cuda.synchronize()
    assert not bool(dn[:N - 1].any())
    assert torch.equal(got, act)
    a = act.cpu().numpy()
    assert 0 < a.sum() < a.size, "degenerate case: one action only"
    # and both env copies are in the same state
    for x, y in zip(d.state(), [env.istate, env.dstate, env.assigned, env.nh_final, env.nh_pure, env.t_cost,
                                env.n_lock, env.window]):
        assert torch.equal(x, y)


def test_truncated_decode_continues():
    """n_max = 6 and then a continuation call (step = 6, fill) against one call with n_max = N * M."""
    N, M, E, seed = 5, 7, 33, 1
    scenes = host_scenes(N, M, E, seed)
    net = gpu_policy(N, M, seed)
    one = Decode(net, scenes, N, M)
    full = one.run(N * M)
    two = Decode(net, scenes, N, M)
    first = two.run(6)
    assert bool(((two.fin == 0) & (two.steps == 6)).any()), "no env was cut at the first call's end"
    assert not bool((two.steps > 6).any())
    second = two.run(N * M)
    assert torch.equal(torch.cat([first, second])[:N * M], full)
    assert bool((second[N * M - 6:] == -1).all())
    assert torch.equal(two.steps, one.steps) and torch.equal(two.fin, one.fin)
    assert bool((two.fin == 1).all())
    assert torch.equal(two.ret, one.ret)
    for x, y in zip(two.state(), one.state()):
        assert torch.equal(x, y)


def _select_np(env, K):
    from uavhip import _lib
    ist = env.istate.cpu().numpy()
    return select_best_np(ist[:, _lib.IST["UAV_IDX"]], env.dstate[:, _lib.DST["J"]].cpu().numpy(),
                          ist[:, _lib.IST["N_COVERED"]], env.assigned.cpu().numpy(), env.tgt_id.cpu().numpy(),
                          env.N, K)


def test_best_of_k():
    N, M, S, K, seed = 5, 7, 8, 4, 1
    scenes = host_scenes(N, M, S, seed)
    net = gpu_policy(N, M, seed)
    rep = tuple(s for s in scenes for _ in range(K))  # scene-major: e = s * K + k
    d = Decode(net, rep, N, M)
    trace = d.run(N * M, greedy_stride=K, seed=3, offset=0, stride=S * K)
    check_against_oracle(d, rep, N, M, trace.cpu().numpy())
    best, J, cov, asg = d.env.select_best(K)
    torch.cuda.synchronize()
    b_np, J_np, c_np, a_np = _select_np(d.env, K)
    assert np.array_equal(best.cpu().numpy(), b_np)
    assert np.array_equal(J.cpu().numpy(), J_np)
    assert np.array_equal(cov.cpu().numpy(), c_np)
    assert np.array_equal(asg.cpu().numpy(), a_np)
    rJ = d.env.dstate[:, 1].view(S, K)
    assert bool((J >= rJ[:, 0]).all())
    # replica 0 is the K = 1 greedy decode of the same scenes
    g = Decode(net, scenes, N, M)
    gt = g.run(N * M, greedy_stride=1)
    assert torch.equal(trace.view(N * M, S, K)[:, :, 0], gt)
    print("best replica per scene:", b_np.tolist(), "J", J_np.round(4).tolist(), "greedy J", rJ[:, 0].cpu().numpy().round(4).tolist())
    assert (b_np > 0).any(), "no scene picked a sampled replica: choose another sampling seed"
    # no replica finished (a decode cut before any episode can end): -1 and nothing assigned
    cut = Decode(net, rep, N, M)
    cut.run(N - 1, greedy_stride=K, optional=False)
    best, J, cov, asg = cut.env.select_best(K)
    assert bool((best == -1).all()) and bool((J == 0).all()) and bool((cov == 0).all()) and bool((asg == -1).all())
    assert bool((cut.fin == 0).all()) and bool((cut.steps == N - 1).all()) and bool((cut.ret == 0).all())
    # ... and decoded on without the optional outputs, its greedy replicas end where the traced decode's
    # ended (the sampled ones drew other numbers: the continuation's counters start again at `offset`)
    cut.run(N * M, greedy_stride=K, optional=False)
    assert bool((cut.fin == 1).all())
    assert torch.equal(cut.steps.view(S, K)[:, 0], d.steps.view(S, K)[:, 0])
    for x, y in zip(cut.state(), d.state()):
        assert torch.equal(x[::K], y[::K])


def test_allocation_solver_end_to_end(scenes_npz):
    from uavhip import AllocationSolver, RolloutEngine, VecUAVEnv
    from uavhip.config import cfg, params_vector
    N, M, K = 16, 32, 4
    fx = [sub(scenes_npz, c["key"]) for c in cases(scenes_npz) if (c["N"], c["M"]) == (N, M)][:4]
    assert len(fx) == 4 and all(np.array_equal(s["params"], params_vector(cfg)) for s in fx)
    net = gpu_policy(N, M, 1)
    # a training engine on the same policy, before the solver exists
    tenv = VecUAVEnv(32, N, M, 1, 1, seed=4)
    eng = RolloutEngine(tenv, net, 8, seed=6)

    def iteration():
        tenv.istate.zero_()
        eng.counter.zero_()
        eng.start()
        tr = eng.collect(eager=True)
        torch.cuda.synchronize()
        return tr.actions.clone(), tr.rewards.clone()

    before = iteration()
    solver = AllocationSolver(net, N, M, samples=K)
    r = solver.solve(scenes=fx, seed=2, trace=True)
    torch.cuda.synchronize()
    c = r.cpu()
    assert c.assignment.shape == (4, N) and c.replica_J.shape == (4, K) and c.actions.shape == (N * M, 4 * K)
    assert bool((c.best_replica >= 0).all())
    for s in range(4):
        e = s * K + int(c.best_replica[s])
        _, _, J_o, cov_o, asg_o, end = oracle_replay(fx[s], c.actions[:, e].numpy(), int(c.steps[s]))
        assert end == int(c.steps[s])
        assert list(c.assignment[s].numpy()) == list(asg_o)
        assert int(c.covered[s]) == cov_o
        assert abs(float(c.J[s]) - J_o) <= RTOL_J * max(1.0, abs(J_o))
        assert float(c.J[s]) == float(c.replica_J[s].max())
    # on-device scenes: the same seed gives the same result; another size resizes the solver
    a = solver.solve(num_scenes=8, seed=5).cpu()
    b = solver.solve(num_scenes=8, seed=5).cpu()
    for x, y in zip((a.assignment, a.J, a.covered, a.best_replica, a.steps, a.replica_J),
                    (b.assignment, b.J, b.covered, b.best_replica, b.steps, b.replica_J)):
        assert torch.equal(x, y)
    assert bool((a.best_replica >= 0).all()) and len(set(a.J.tolist())) > 1
    # the training engine collects the same trajectory after the solves
    after = iteration()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
