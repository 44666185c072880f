"""The actor-only step's pruned attention in the projection's registers (one wave per head,
encoder_layer_rows ONEPASS, in k_rollout_actor_steps and k_decode_steps). Marked gpu.

The lane mapping can go wrong in four ways, one test each: a padding mask read for the wrong sample or
position (every count of masked rows, bitwise against the pinned one-kernel engine); a head taken from
the wrong wave (a policy whose heads are scaled apart, against oracle/policy_ref.py); the decode kernel's
copy of the block (against the same envs stepped one launch at a time); a ring value dropped on its way
to the scores (a +inf key row must reach the log-prob)."""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# (E, N, M, T, full_reset_period): a partial last workgroup, one env per wave, an episode ends every few
# steps; the grouped env path with full windows
SHAPES = [(17, 4, 4, 9, 3), (34, 16, 32, 6, 0)]
ENV_STATE = ("istate", "dstate", "window", "nh_final", "nh_pure", "t_cost", "n_lock", "assigned")
TRAJ = ("obs", "actions", "logp", "rewards", "dones", "info", "values", "last_values", "ret", "adv")
ACTOR_ROW = 2 * 128      # a ring row: actor K | V, then critic Q | K | V (policy_encoder.hpp kRowFloats)
POS_TABLE = 2 * 5 * 384  # the Win pos_s table in front of the ring (policy_encoder.hpp kPposFloats)
# against torch fp32: the bar of test_gpu_value_pass.test_deferred_values_match_pinned_torch_and_gae
RTOL, ATOL = 1e-5, 1e-5


@functools.lru_cache(maxsize=None)
def _runs(shape):
    """Two iterations of the pinned engine (persistent=True: k_rollout_steps) and of a default (deferred)
    engine on the same seeds -> per engine: every output of every iteration, env state, actor ring rows."""
    from uavhip.policy import TransformerActorCritic
    from uavhip.rollout import RolloutEngine
    from uavhip.vec_env import VecUAVEnv
    E, N, M, T, period = shape
    torch.manual_seed(0)
    pol = TransformerActorCritic().cuda()
    out = []
    for pinned in (True, False):
        env = VecUAVEnv(E, N, M, 1, 1, seed=6, full_reset_period=period)
        eng = RolloutEngine(env, pol, T, seed=5, **(dict(persistent=True) if pinned else {}))
        assert eng.persistent and eng.deferred_value == (not pinned)
        eng.start()
        its = []
        for _ in range(2):
            tr = eng.collect()
            its.append({k: getattr(tr, k).clone() for k in TRAJ})
        assert int((env.errors() & 1).max()) == 0
        ring = eng.rowproj[POS_TABLE:].view(5, E, 640)
        out.append(dict(its=its, env={k: getattr(env, k).clone() for k in ENV_STATE},
                        actor_rows=ring[:, :, :ACTOR_ROW].clone()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_deferred_engine_is_bitwise_the_pinned_engine(shape):
    pin, dfr = _runs(shape)
    for it, (a, b) in enumerate(zip(pin["its"], dfr["its"])):
        for k in TRAJ:
            assert torch.equal(a[k], b[k]), (it, k)
    for k in ENV_STATE:
        assert torch.equal(pin["env"][k], dfr["env"][k]), k
    assert torch.equal(pin["actor_rows"], dfr["actor_rows"])


def test_every_mask_count_occurs():
    """A condition of the cases above, not a measurement: over the compared windows, every number of
    all-zero (padding) rows among positions 0-3 occurs -- 0, 1, 2, 3 and 4."""
    seen = set()
    for shape in SHAPES:
        _, dfr = _runs(shape)
        for it in dfr["its"]:
            obs = it["obs"].cpu().numpy()  # [T + 1][E][5][14]
            zero = (np.abs(obs[:, :, :4, :]).sum(-1) == 0).sum(-1)
            seen |= set(int(c) for c in np.unique(zero))
    assert seen == {0, 1, 2, 3, 4}, seen


def _head_scaled_policy():
    """Every head of the actor's layer 0 and of the critic's layer 1 scaled apart: the in_proj rows (and
    bias) of head h times 1 + h / 4, in Q, K and V. The actor head's last layer gets weights of 0.25 randn:
    its 0.01 initial gain would hide the trunk from the log-probs, and at randn itself the logits reach
    +-15, where torch fp32's own error against fp64 (8e-6 on the CPU) leaves the bar no room. At 0.25 the
    reference is within 1.6e-6 of fp64, and one head's K rows at a neighbour's scale move logp by 7e-4."""
    from uavhip.policy import TransformerActorCritic
    torch.manual_seed(3)
    net = TransformerActorCritic()
    f = (1.0 + torch.arange(8, dtype=torch.float32) / 4).repeat_interleave(16).repeat(3)  # [384]
    with torch.no_grad():
        for attn in (net.actor_net.transformer.layers[0].self_attn, net.critic_net.transformer.layers[1].self_attn):
            attn.in_proj_weight.mul_(f[:, None])
            attn.in_proj_bias.mul_(f)
        net.actor_head[2].weight.copy_(0.25 * torch.randn(2, 64, generator=torch.Generator().manual_seed(3)))
    return net


@pytest.mark.parametrize("E", [16, 19])
def test_all_heads_against_policy_ref(E):
    """One workgroup, and one with a partial tail: per-sample logp of the actor step and values of
    value_steps against oracle/policy_ref.py (torch fp32 on the CPU) on the recorded windows. The
    reference itself is held to the same bar against its fp64 evaluation of this policy."""
    from oracle import policy_ref
    from uavhip.rollout import RolloutEngine
    from uavhip.vec_env import VecUAVEnv
    cpu = _head_scaled_policy()
    T = 6
    env = VecUAVEnv(E, 4, 4, 1, 1, seed=6, full_reset_period=3)
    eng = RolloutEngine(env, copy.deepcopy(cpu).cuda(), T, seed=5)
    assert eng.deferred_value
    eng.start()
    eng.collect()
    tr = eng.collect()  # the second iteration: windows of every fill level
    torch.cuda.synchronize()
    x = tr.obs.reshape((T + 1) * E, 5, 14).cpu()
    a = torch.cat([tr.actions.reshape(-1).long().cpu(), torch.zeros(E, dtype=torch.long)])
    sd = {k: v.detach() for k, v in cpu.state_dict().items()}
    logp, value, _, _ = policy_ref.evaluate(sd, x, a)
    lp64, v64, _, _ = policy_ref.evaluate({k: v.double() for k, v in sd.items()}, x.double(), a)
    torch.testing.assert_close(logp, lp64.float(), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(value, v64.float(), rtol=RTOL, atol=ATOL)
    got_lp = tr.logp.reshape(-1).cpu()
    got_v = torch.cat([tr.values, tr.last_values[None]]).reshape(-1).cpu()
    print(f"E={E}: max |logp - ref| {float((got_lp - logp[:T * E]).abs().max()):.3e}, "
          f"max |value - ref| {float((got_v - value).abs().max()):.3e}; logp spread {float(logp.std()):.3f}")
    torch.testing.assert_close(got_lp, logp[:T * E], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(got_v, value, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("greedy", [True, False])
def test_decode_equals_single_steps(greedy):
    """uavhip_decode_steps on (E, N, M) = (19, 8, 16) against identical env copies stepped one launch at
    a time: actions, step counts and returns equal. Sampled: uavhip_rollout_step with the decode's seed,
    offset and stride. Greedy (uavhip_rollout_step only samples): the arg-max of uavhip_policy_forward_rows'
    logits, then uavhip_env_step. A finished env reports a zero window, reward 0 and done in both."""
    from test_gpu_solve import Decode, gpu_policy, host_scenes, make_env
    from uavhip.policy import rowproj_buffer
    E, N, M, seed = 19, 8, 16, 1
    n_max, off, stride = N * M, 1000, E + 3
    scenes = host_scenes(N, M, E, seed)
    net = gpu_policy(N, M, seed)
    d = Decode(net, scenes, N, M)
    trace = d.run(n_max, greedy_stride=1 if greedy else 0, seed=5, offset=off, stride=stride).cpu().numpy()
    env = make_env(scenes, N, M)
    dev = env.device
    rp = rowproj_buffer(E, dev)
    obs = torch.zeros(E, 5, 14, device=dev)
    env.reset(episode=1, obs_out=obs)
    acts, rews, dns = [], [], []
    for t in range(n_max):
        act = torch.empty(E, dtype=torch.int8, device=dev)
        rew = torch.empty(E, dtype=torch.float64, device=dev)
        dn = torch.empty(E, dtype=torch.uint8, device=dev)
        nxt = torch.empty_like(obs)
        if greedy:
            logits = torch.empty(E, 2, device=dev)
            net.fused_forward(obs, logits=logits, rowproj=rp, step=t, fill=t == 0, check_weights=False)
            act = (logits[:, 1] > logits[:, 0]).to(torch.int8)
            env.step(act, auto_reset=False, obs_out=nxt, reward_out=rew, done_out=dn, want_info=False)
        else:
            net.rollout_step(env, obs, rp, t, t == 0, act, torch.empty(E, device=dev), torch.empty(E, device=dev), nxt,
                             rew, dn, auto_reset=False, seed=5, offset=off + t * stride)
        acts.append(act)
        rews.append(rew)
        dns.append(dn)
        obs = nxt
    a, r, dn = (torch.stack(v).cpu().numpy() for v in (acts, rews, dns))
    steps, ret = d.steps.cpu().numpy(), d.ret.cpu().numpy()
    assert bool((d.fin == 1).all()) and bool(dn[-1].all())
    for e in range(E):
        n = int(np.argmax(dn[:, e] != 0)) + 1
        assert steps[e] == n, (e, steps[e], n)
        assert np.array_equal(trace[:n, e], a[:n, e]) and (trace[n:, e] == -1).all(), e
        s = 0.0
        for t in range(n):
            s = s + r[t, e]
        assert ret[e] == s, (e, ret[e], s)
    assert 0 < a[dn.cumsum(0) - dn == 0].sum() < steps.sum(), "degenerate case: one action only"
    assert len(set(steps.tolist())) > 1, "degenerate case: every episode has the same length"


def test_actor_step_non_finite_ring_row_stays_non_finite():
    """A +inf feature in a key row that the actor step reads from the ring makes that sample's logp
    non-finite, at every step whose window holds the row, and leaves every other sample's logp what it was
    (test_value_steps_non_finite_rows_stay_non_finite's pattern). Five warm-up steps fill the windows; the
    row is position 3 of the next launch's first windows, so fill projects it into the ring and the launch's
    three steps read it there as key position 3, 2 and 1 (no episode of 8 UAVs ends before its 8th step).
    In the first step the row is also in the workgroup's windows: layer 0's attention scale is one per
    workgroup, so its other 15 samples are not compared there."""
    from test_gpu_solve import gpu_policy, host_scenes, make_env
    from uavhip.policy import rowproj_buffer
    E, N, M, seed, warm, n = 35, 8, 16, 1, 5, 3
    scenes = host_scenes(N, M, E, seed)
    net = gpu_policy(N, M, seed)
    logps = []
    for poison in (False, True):
        env = make_env(scenes, N, M)
        dev = env.device

        def launch(obs, step, k):
            act = torch.empty(k, E, dtype=torch.int8, device=dev)
            lp = torch.empty(k, E, device=dev)
            rew = torch.empty(k, E, dtype=torch.float64, device=dev)
            dn = torch.empty(k, E, dtype=torch.uint8, device=dev)
            net.rollout_actor_steps(env, obs, rowproj_buffer(E, dev), step, True, act, lp, rew, dn, None, seed=5,
                                    offset=step * E, offset_stride=E)
            assert not bool(dn[:max(0, N - 1 - step)].any())  # the 8th step may end an episode, none before
            return lp

        obs = torch.zeros(warm + 1, E, 5, 14, device=dev)
        env.reset(episode=1, obs_out=obs[0])
        launch(obs, 0, warm)
        obs2 = torch.zeros(n + 1, E, 5, 14, device=dev)
        obs2[0] = obs[warm]
        assert bool((obs2[0].abs().sum(-1) > 0).all()), "a padding row is left after the warm-up"
        if poison:
            obs2[0, :3, 3, 3] = float("inf")
        logps.append(launch(obs2, warm, n).clone())
    torch.cuda.synchronize()
    base, got = logps
    assert bool(torch.isfinite(base).all())
    assert not torch.isfinite(got[:, :3]).any(), "a log-prob that read the +inf row came out finite"
    assert bool(torch.isfinite(got[1:, 3:]).all()) and bool(torch.isfinite(got[0, 16:]).all())
    assert torch.equal(got[:, 16:], base[:, 16:])  # (the first workgroup's envs may have sampled other actions)
