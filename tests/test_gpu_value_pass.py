"""The rollout with the critic off the step chain: uavhip_rollout_actor_steps (the T steps
on the actor alone) + uavhip_value_steps (the critic over the recorded windows in groups of five
steps, bootstrap included) against uavhip_rollout_steps + uavhip_policy_value_rows. Marked gpu.

Bars: everything the actor launch writes is bitwise k_rollout_steps' (the same code); the values
against the pinned engine's at rtol 1e-5 / atol 2e-6 (the project's bar between two forward paths,
test_rollout_row_cache_matches_full_forward) and against torch `evaluate` of the recorded windows at
rtol 1e-5 / atol 1e-5 (the at-size oracle test's bar, the independent reference); returns bit-exact
and normalised advantages at rtol 1e-5 / atol 2e-6 against oracle/gae.py (test_gae_2d_vs_oracle)."""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# (E, N, M, T, full_reset_period): a partial last workgroup with odd E (one env per wave) and episodes
# of <= 16 steps (resets inside groups); the grouped env path; T + 1 exactly one group; one short group
SHAPES = [(33, 4, 4, 7, 5), (64, 16, 32, 11, 3), (96, 64, 64, 4, 0), (40, 8, 16, 1, 2)]
ENV_STATE = ("istate", "dstate", "window", "nh_final", "nh_pure", "t_cost", "n_lock", "assigned")
ACTOR_ROW = 2 * 128  # a ring row: actor K | V, then critic Q | K | V (policy_encoder.hpp kRowFloats)
POS_TABLE = 2 * 5 * 384  # the Win pos_s table in front of the ring (policy_encoder.hpp kPposFloats)


@functools.lru_cache(maxsize=None)
def _runs(shape):
    """Two iterations of the pinned engine (persistent=True: k_rollout_steps + value_rows) and of a
    default engine (deferred) on the same seeds -> per engine, per iteration, clones of every output.
    (T = 1: 40 iterations -- an episode of 8 UAVs lasts at least 8 steps, and the shape must see one end.)"""
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
        for _ in range(2 if T > 1 else 40):
            tr = eng.collect()
            its.append({k: getattr(tr, k).clone() for k in ("obs", "actions", "logp", "rewards", "dones", "info",
                                                            "values", "last_values", "ret", "adv")})
        assert int((env.errors() & 1).max()) == 0
        ring = eng.rowproj[POS_TABLE:].view(5, E, 640)  # [slot][env][actor K | V, critic Q | K | V]
        out.append(dict(its=its, env={k: getattr(env, k).clone() for k in ENV_STATE},
                        actor_rows=ring[:, :, :ACTOR_ROW].clone(), pos_table=eng.rowproj[:POS_TABLE].clone()))
    torch.cuda.synchronize()
    return pol, out


@pytest.mark.parametrize("shape", SHAPES)
def test_actor_launch_matches_rollout_steps(shape):
    """Windows, actions, logp, rewards, dones, info, the whole env state and the actor's part of the ring
    rows of the deferred engine are bitwise the pinned engine's, over every iteration, with auto-reset."""
    _, (pin, dfr) = _runs(shape)
    for it, (a, b) in enumerate(zip(pin["its"], dfr["its"])):
        for k in ("obs", "actions", "logp", "rewards", "dones", "info"):
            assert torch.equal(a[k], b[k]), (it, k)
    for k in ENV_STATE:
        assert torch.equal(pin["env"][k], dfr["env"][k]), k
    assert torch.equal(pin["actor_rows"], dfr["actor_rows"])
    assert torch.equal(pin["pos_table"], dfr["pos_table"])
    if shape[1] * shape[2] <= 512:
        assert any(bool(it["dones"].any()) for it in dfr["its"])  # episodes ended inside the rollout


@pytest.mark.parametrize("shape", SHAPES)
def test_deferred_values_match_pinned_torch_and_gae(shape):
    from oracle import gae as ogae
    pol, (pin, dfr) = _runs(shape)
    E, T = shape[0], shape[3]
    for it, (a, b) in enumerate(zip(pin["its"], dfr["its"])):
        for k in ("values", "last_values"):
            d = float((a[k] - b[k]).abs().max())
            print(f"{shape} iteration {it} {k}: max |deferred - pinned| {d:.3e}")
            torch.testing.assert_close(b[k], a[k], rtol=1e-5, atol=2e-6)
        with torch.no_grad():
            x = b["obs"].reshape((T + 1) * E, 5, 14)
            _, v_t, _ = pol.evaluate(x, torch.zeros(len(x), dtype=torch.long, device="cuda"))
        v_t = v_t[:, 0].view(T + 1, E)
        print(f"{shape} iteration {it}: max |deferred - torch| {float((torch.cat([b['values'], b['last_values'][None]]) - v_t).abs().max()):.3e}")
        torch.testing.assert_close(b["values"], v_t[:T], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(b["last_values"], v_t[T], rtol=1e-5, atol=1e-5)
        r_o, a_o = ogae.gae_2d(b["rewards"].cpu().numpy(), b["dones"].cpu().numpy(), b["values"].cpu().numpy(),
                               last_values=b["last_values"].cpu().numpy())
        np.testing.assert_array_equal(b["ret"].cpu().numpy(), r_o)
        if T * E > 1:
            np.testing.assert_allclose(b["adv"].cpu().numpy(), ogae.normalize(a_o)[0], rtol=1e-5, atol=2e-6)


def _sequence(B, n, scale, g, pad_envs=16, scaled_rows=6):
    """A deque sequence of n + 1 windows [n + 1][B][5][14] from n + 5 rows: the first `scaled_rows` rows
    times `scale` (so windows 0 .. scaled_rows - 1 mix scaled and O(1) rows), rows 0-3 of the first
    `pad_envs` envs zero (a reset window: four padding rows and the new row)."""
    rows = torch.randn(n + 5, B, 14, generator=g) * 0.7
    rows[:scaled_rows] *= scale
    rows[:4, :pad_envs] = 0
    return rows


def _windows(rows):
    n = rows.shape[0] - 5
    return torch.stack([rows[t:t + 5].transpose(0, 1) for t in range(n + 1)]).contiguous().cuda()


@pytest.mark.parametrize("case", ["inputs x1e5", "inputs x1e-6", "ffn1 x4e4"])
def test_value_steps_out_of_fp16_range_matches_torch(policy_npz, case):
    """The window cases of test_rollout_steps_out_of_fp16_range_matches_torch (rows x 1e5 and x 1e-6 mixed
    with O(1) rows; the critic's FFN1 x 4e4) through uavhip_value_steps itself, three workgroups, two
    full groups and a short one: values against torch `evaluate` at that test's own bar -- 1e-5
    relative, or no further from the fp64 forward than twice torch fp32's worst error on the case."""
    import copy
    from test_gpu_policy_gae import _load_policy, _range_case
    from uavhip.policy import rowproj_buffer
    net = _load_policy(policy_npz, "b")
    xs = _range_case(net, case)
    B, n = 48, 11
    obs = _windows(_sequence(B, n, xs, torch.Generator().manual_seed(21)))
    val, last = torch.empty(n, B, device="cuda"), torch.empty(B, device="cuda")
    net.value_steps(obs, rowproj_buffer(B), 0, val, last, fill=True)
    got = torch.cat([val, last[None]]).reshape(-1).double().cpu()
    assert torch.isfinite(got).all(), "non-finite output"
    x = obs.reshape(-1, 5, 14)
    a = torch.zeros(len(x), dtype=torch.long, device="cuda")
    with torch.no_grad():
        _, v_t, _ = net.evaluate(x, a)
        _, v_64, _ = copy.deepcopy(net).double().cpu().evaluate(x.double().cpu(), a.cpu())
    f32, f64 = v_t[:, 0].double().cpu(), v_64[:, 0]
    atol = 1e-5 * max(1.0, float(v_t.abs().max()))
    bar = 1e-5 * f32.abs() + atol
    e_hip, e_t32 = (got - f64).abs(), (f32 - f64).abs()
    near = (got - f32).abs() <= bar
    ok = near | (e_hip <= 2 * float(e_t32.max()) + atol)
    print(f"{case}: max |HIP - torch fp32| / bar {float(((got - f32).abs() / bar).max()):.3e} ({int((~near).sum())} of "
          f"{near.numel()} beyond); vs fp64: HIP max {float(e_hip.max()):.3e}, torch fp32 max {float(e_t32.max()):.3e}")
    assert bool(ok.all()), f"{case}: {int((~ok).sum())} values beyond both bars"


def test_value_steps_non_finite_rows_stay_non_finite(policy_npz):
    """A row beyond every number format's range (+inf in one feature) makes every value that reads it
    non-finite -- as a query row and as a key row from the ring, in the per-window front and through
    the batched tail -- and leaves every value of another window or workgroup what it was (layer 0's
    attention scale is one per workgroup, so the 16 envs of the row's workgroup share its fate)."""
    from test_gpu_policy_gae import _load_policy
    from uavhip.policy import rowproj_buffer
    net = _load_policy(policy_npz, "b")
    B, n = 48, 11
    rows = _sequence(B, n, 1.0, torch.Generator().manual_seed(22))
    val0, last0 = torch.empty(n, B, device="cuda"), torch.empty(B, device="cuda")
    net.value_steps(_windows(rows), rowproj_buffer(B), 0, val0, last0, fill=True)
    rows[7, :8, 3] = float("inf")  # the newest row of window 3, a key row of windows 4 .. 7, of envs 0 .. 7
    val, last = torch.empty(n, B, device="cuda"), torch.empty(B, device="cuda")
    net.value_steps(_windows(rows), rowproj_buffer(B), 0, val, last, fill=True)
    assert not torch.isfinite(val[3:8, :8]).any(), "a value that read the +inf row came out finite"
    same = torch.ones(n, B, dtype=torch.bool, device="cuda")
    same[3:8, :16] = False
    assert torch.equal(val[same], val0[same]) and torch.equal(last, last0)


def test_deferred_rollout_graph_replay_matches_eager():
    """In deferred mode the captured hipGraph iteration (the value pass is one more node) reproduces
    eager launches bit for bit over three iterations, with a weight change in between
    (test_rollout_graph_replay_matches_eager's pattern)."""
    from uavhip.policy import TransformerActorCritic
    from uavhip.rollout import RolloutEngine
    from uavhip.vec_env import VecUAVEnv
    outs = []
    for graph in (False, True):
        torch.manual_seed(0)
        env = VecUAVEnv(256, 8, 16, 1, 1, seed=3, full_reset_period=2)
        pol = TransformerActorCritic().cuda()
        eng = RolloutEngine(env, pol, 16, seed=4)
        assert eng.deferred_value
        eng.start()
        if graph:
            eng.capture()
            eng.counter.zero_()
            # capture ran the body once on a side stream: rewind the device state
            env2 = VecUAVEnv(256, 8, 16, 1, 1, seed=3, full_reset_period=2)
            env2.istate[:, 4] = 1
            env2.generate_scenes()
            for name in ("nh_final", "nh_pure", "t_cost", "n_lock", "assigned", "istate", "dstate", "window"):
                getattr(env, name).copy_(getattr(env2, name))
            for k in env._scene:
                env._scene[k].copy_(env2._scene[k])
            env.reset(episode=1, obs_out=eng.traj.obs[eng.T])
        res = []
        for it in range(3):
            if it == 1:
                with torch.no_grad():
                    pol.critic_head[2].bias.add_(0.5)   # weights change between iterations
                    pol.actor_head[2].bias.add_(0.5)
            tr = eng.collect()
            torch.cuda.synchronize()
            res.append([x.clone() for x in (tr.actions, tr.logp, tr.rewards, tr.dones, tr.obs, tr.values,
                                            tr.last_values, tr.ret, tr.adv)])
        outs.append(res)
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
