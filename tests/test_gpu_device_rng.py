"""GPU: the two on-device random decisions that feed training, pinned to the host restatement
tests/device_rng.py (checked on the CPU by tests/test_device_rng_host.py).

Scenes: VecUAVEnv.generate_scenes / refresh_scenes / the spare flip of the step kernels against
scene_np, every env of the launch, under the counter contract of include/uavhip.h ("Scene counters" at
uavhip_scene_generate). Integer fields, values, costs, loads and positions bitwise; the two velocity
fields (cos / sin of the device's libm times a speed) within 5 np.spacing of the correctly rounded
product: 4 ulp for the device's cos / sin (the OpenCL bound ocml is built to) plus 1 for the product.

Sampling: every draw of every entry point against sample_uniform under the counter contract of
include/uavhip.h ("Sampling counter" at uavhip_policy_forward). A draw is decided when |u - p0| >
DELTA = 2e-6 (the kernel's fp32 p0 = expf(l0 - lse) carries a few fp32 ulp of O(1), about 5e-7; u is
exact); a decided draw's action must be 0 iff u < p0, at most one draw of a case may be undecided.
Every case also asserts its own power: at least a quarter of its draws have 0.2 <= p0 <= 0.8, and on
the same device outputs the restatement with every counter moved by +1, and with the seed's high word
cleared, disagrees with the device on at least 20 % of the decided draws.

Measured on an MI355X (the tests print these; each test's docstring has its own figures): every
bitwise field bitwise in every scene compared, velocities within 2 np.spacing; 0 undecided and 0 wrong
draws in every sampling case, the controls' disagreement between 0.28 and 0.56."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from device_rng import FIELDS, SCENE_SHAPES, sample_uniform, scene_np

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

SEED = 2024
SEED_HI = (0xDEADBEEF << 32) | 7   # a key whose high word matters
BITWISE = ("uav_type", "tgt_id", "tgt_value", "uav_cost", "uav_load", "uav_pos", "tgt_pos", "tgt_vel", "nfz_pos",
           "icp_pos")
VELOCITY = ("uav_vel", "icp_vel")
VEL_ULP = 5.0
DELTA = 2e-6
SMALL = (4, 4, 1, 1, 9)


# ------------------------------------------------------------------ scenes
def _env(N, M, Kn, Ki, E, seed=SEED, **kw):
    from uavhip.vec_env import VecUAVEnv
    kw.setdefault("full_reset_period", 0)
    return VecUAVEnv(E, N, M, Kn, Ki, seed=seed, **kw)


def _gen_vector(v):
    from uavhip.config import gen_vector
    return gen_vector(v.cfg)


def _storage(v):
    """Every scene array as stored, [B * E, ...] (row sel * E + e), and istate [E, IST_COUNT]."""
    torch.cuda.synchronize()
    return {k: v._scene[k].cpu().numpy() for k in FIELDS}, v.istate.cpu().numpy()


class _Worst:
    """The largest velocity error seen, in np.spacing units of the expected value."""
    def __init__(self):
        self.ulp = 0.0


def _compare_row(tag, st, row, want, v, worst):
    """Storage row `row` against the restated scene `want`."""
    n = dict(nfz_pos=v.Kn, icp_pos=v.Ki, icp_vel=v.Ki)  # the arrays hold max(K, 1) rows
    for k in BITWISE:
        got = st[k][row][:n.get(k, None)]
        assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), (tag, k, got, want[k])
    for k in VELOCITY:
        got = st[k][row][:n.get(k, None)]
        if got.size == 0:
            continue
        err = np.abs(got - want[k]) / np.spacing(np.abs(want[k]))
        worst.ulp = max(worst.ulp, float(err.max()))
        assert float(err.max()) <= VEL_ULP, (tag, k, float(err.max()), got, want[k])


def _compare_env(tag, v, st, e, gen, worst, buffer=None, seed=None):
    """Env e's scene in `buffer` (default: its active one) against generation `gen`."""
    scenes, ist = st
    from uavhip import _lib
    sel = int(ist[e, _lib.IST["SCENE_SEL"]]) & 1 if v.B == 2 else 0
    b = sel if buffer is None else buffer
    want = scene_np(v.desc.seed if seed is None else seed, v.env_base + e, gen, v.N, v.M, v.Kn, v.Ki, _gen_vector(v))
    _compare_row((tag, e, gen, b), scenes, b * v.E + e, want, v, worst)


def _scene_gen(st):
    from uavhip import _lib
    return st[1][:, _lib.IST["SCENE_GEN"]]


@pytest.mark.parametrize("N,M,Kn,Ki,E", SCENE_SHAPES)
def test_generated_scenes_are_the_restatement(N, M, Kn, Ki, E):
    """generate_scenes() on a single-buffered env: scene 0 of every env, SCENE_GEN = 1.
    Measured on an MI355X: every bitwise field bitwise at all seven shapes; the largest velocity error
    1 np.spacing (at 4 x 4 and 16 x 32; 0 at the other five shapes)."""
    v = _env(N, M, Kn, Ki, E)
    v.generate_scenes()
    st = _storage(v)
    worst = _Worst()
    for e in range(E):
        _compare_env("generate", v, st, e, 0, worst)
    assert (_scene_gen(st) == 1).all()
    print(f"{N} x {M}, Kn {Kn}, Ki {Ki}, E {E}: largest velocity error {worst.ulp:.3f} np.spacing (bar {VEL_ULP})")


def test_velocity_error_is_reported():
    """The largest |device - want| / np.spacing(|want|) of uav_vel and icp_vel over 512 envs of 16 x 32
    with 8 interceptors (12,288 cos / sin pairs). Measured on an MI355X: 2.000 np.spacing."""
    v = _env(16, 32, 1, 8, 512)
    v.generate_scenes()
    st = _storage(v)
    worst = _Worst()
    for e in range(512):
        _compare_env("velocity", v, st, e, 0, worst)
    print(f"largest velocity error {worst.ulp:.3f} np.spacing (bar {VEL_ULP})")
    assert worst.ulp <= VEL_ULP


def test_seed_high_word_env_base_and_weather():
    """One small shape each: a key with a non-zero high word; env_base = 1000 (the counter's env word
    is env_base + e); weather factors away from 1 (at 1.0 a swapped factor is invisible)."""
    from uavhip.config import Config
    worst = _Worst()
    v = _env(*SMALL, seed=SEED_HI)
    v.generate_scenes()
    st = _storage(v)
    for e in range(v.E):
        _compare_env("seed high word", v, st, e, 0, worst, seed=SEED_HI)
    v = _env(*SMALL, env_base=1000)
    v.generate_scenes()
    st = _storage(v)
    for e in range(v.E):
        _compare_env("env_base", v, st, e, 0, worst)
    c = Config()
    c.WEATHER_SPEED_FACTOR, c.WEATHER_LOAD_FACTOR = 0.8, 0.9
    v = _env(*SMALL, config=c)
    v.generate_scenes()
    st = _storage(v)
    assert set(np.unique(st[0]["uav_load"])) == {0.95 * 0.9, 1.0 * 0.9}
    for e in range(v.E):
        _compare_env("weather", v, st, e, 0, worst)
    print(f"largest velocity error {worst.ulp:.3f} np.spacing")


def test_mask_and_second_generation():
    """A masked generate_scenes() leaves the other envs' scene and SCENE_GEN alone; a second call draws
    generation gen + 1 -- with two buffers gen + 2 into the active buffer and gen + 3 into the spare,
    after 0 and 1 (both buffers read through the [2][E] storage)."""
    worst = _Worst()
    v = _env(*SMALL)
    E = v.E
    v.generate_scenes()
    mask = torch.zeros(E, dtype=torch.uint8, device="cuda")
    mask[[1, 4, 8]] = 1
    v.generate_scenes(mask)
    st = _storage(v)
    m = mask.cpu().numpy().astype(bool)
    for e in range(E):
        _compare_env("mask", v, st, e, 1 if m[e] else 0, worst)
    assert (_scene_gen(st) == np.where(m, 2, 1)).all()
    v.generate_scenes()
    st = _storage(v)
    for e in range(E):
        _compare_env("second", v, st, e, 2 if m[e] else 1, worst)
    assert (_scene_gen(st) == np.where(m, 3, 2)).all()

    v = _env(*SMALL, scene_buffers=2)
    v.generate_scenes()
    st = _storage(v)
    for e in range(E):
        _compare_env("two buffers", v, st, e, 0, worst, buffer=0)
        _compare_env("two buffers", v, st, e, 1, worst, buffer=1)
    assert (_scene_gen(st) == 2).all()
    v.generate_scenes(mask)
    st = _storage(v)
    for e in range(E):
        _compare_env("two buffers, second", v, st, e, 2 if m[e] else 0, worst, buffer=0)
        _compare_env("two buffers, second", v, st, e, 3 if m[e] else 1, worst, buffer=1)
    assert (_scene_gen(st) == np.where(m, 4, 2)).all()


LIFE = (2, 2, 1, 1, 6)


def _check_lifecycle(tag, v, k, worst):
    """Every env's active scene is generation k[e], its spare generation k[e] + 1 and fresh."""
    from uavhip import _lib
    st = _storage(v)
    ist = st[1]
    assert (ist[:, _lib.IST["ERROR"]] == 0).all(), (tag, ist[:, _lib.IST["ERROR"]])
    assert (ist[:, _lib.IST["SCENE_STALE"]] == 0).all(), tag
    assert (_scene_gen(st) == k + 2).all(), (tag, _scene_gen(st), k)
    for e in range(v.E):
        sel = int(ist[e, _lib.IST["SCENE_SEL"]]) & 1
        assert sel == k[e] % 2, (tag, e, sel, k[e])
        _compare_env(tag, v, st, e, int(k[e]), worst)
        _compare_env(tag, v, st, e, int(k[e]) + 1, worst, buffer=sel ^ 1)


def test_scene_lifecycle_through_env_steps():
    """full_reset_period = 1, two buffers, all-assign steps with auto_reset and a refresh after every
    step: after its k-th episode env e stands on scene_np(seed, env_base + e, k), k = 0, 1, 2, ... in
    order -- none skipped, none seen twice -- and SCENE_GEN is k + 2 (the spare holds k + 1).
    Measured on an MI355X: every env reaches generation 5 in 10 steps, every comparison bitwise."""
    v = _env(*LIFE, seed=SEED_HI, full_reset_period=1, env_base=40)
    E = v.E
    v.generate_scenes()
    v.reset(episode=1)
    worst = _Worst()
    k = np.zeros(E, np.int64)
    _check_lifecycle("start", v, k, worst)
    ones = torch.ones(E, dtype=torch.int8, device="cuda")
    for step in range(5 * v.N * v.M):
        _, _, done, _ = v.step(ones, auto_reset=True)
        k += done.cpu().numpy().astype(np.int64)
        v.refresh_scenes()
        _check_lifecycle(("step", step), v, k, worst)
        if k.min() >= 5:
            break
    print(f"generations reached per env {k.tolist()} in {step + 1} steps")
    assert k.min() >= 5


@pytest.mark.parametrize("path", ["rollout_steps", "rollout_actor_steps"])
def test_scene_lifecycle_through_the_persistent_rollout(path):
    """The same through RolloutEngine's one-launch iteration (the flip inside k_rollout_steps /
    k_rollout_actor_steps, the refresh at the iteration's end). T = 2 = N: an episode takes at least
    two steps, so an env flips at most once between two refreshes."""
    from uavhip.policy import TransformerActorCritic
    from uavhip.rollout import RolloutEngine
    torch.manual_seed(3)
    net = TransformerActorCritic().cuda()
    v = _env(*LIFE, seed=SEED_HI, full_reset_period=1, env_base=40)
    kw = dict(persistent=True) if path == "rollout_steps" else {}
    eng = RolloutEngine(v, net, 2, seed=11, total_envs=64, **kw)
    assert eng.persistent and eng.deferred_value == (path == "rollout_actor_steps")
    eng.start()
    worst = _Worst()
    k = np.zeros(v.E, np.int64)
    _check_lifecycle("start", v, k, worst)
    for it in range(16):
        tr = eng.collect()
        torch.cuda.synchronize()
        ends = tr.dones.cpu().numpy().astype(np.int64).sum(0)
        assert ends.max() <= 1
        k += ends
        _check_lifecycle((path, it), v, k, worst)
    print(f"{path}: generations reached per env {k.tolist()}")
    assert k.min() >= 4


# ------------------------------------------------------------------ sampling
def _p0_of_logits(lg):
    lg = np.asarray(lg, np.float64)
    return 1.0 / (1.0 + np.exp(lg[..., 1] - lg[..., 0]))


def _p0_of_logp(actions, logp):
    p = np.exp(np.asarray(logp, np.float64))
    return np.where(np.asarray(actions) == 0, p, 1.0 - p)


def _check_draws(tag, seed, counters, actions, p0, unique=True):
    """Every draw of one case: counters (Python ints), the device's actions and p0, flattened alike."""
    counters = [int(c) for c in np.ravel(np.asarray(counters, dtype=object))]
    actions = np.ravel(np.asarray(actions)).astype(np.int64)
    p0 = np.ravel(np.asarray(p0, np.float64))
    n = len(counters)
    assert actions.shape == p0.shape == (n,) and set(np.unique(actions)) <= {0, 1}
    if unique:
        assert len(set(c & (2 ** 64 - 1) for c in counters)) == n, (tag, "a counter occurs twice")
    u = sample_uniform(seed, counters)
    decided = np.abs(u - p0) > DELTA
    want = np.where(u < p0, 0, 1)
    wrong = decided & (actions != want)
    mid = float(((p0 >= 0.2) & (p0 <= 0.8)).mean())
    shifted = np.where(sample_uniform(seed, [c + 1 for c in counters]) < p0, 0, 1)
    low_key = np.where(sample_uniform(int(seed) & 0xFFFFFFFF, counters) < p0, 0, 1)
    off1 = float((shifted != actions)[decided].mean())
    off2 = float((low_key != actions)[decided].mean())
    print(f"{tag}: {int(decided.sum())} decided, {int((~decided).sum())} undecided, {int(wrong.sum())} wrong; "
          f"share with 0.2 <= p0 <= 0.8: {mid:.3f}; disagreement of the controls: counter + 1 {off1:.3f}, "
          f"seed high word cleared {off2:.3f}")
    assert not wrong.any(), (tag, np.nonzero(wrong)[0][:8], u[wrong][:8], p0[wrong][:8], actions[wrong][:8])
    assert int((~decided).sum()) <= 1, tag
    assert mid >= 0.25, tag
    assert off1 >= 0.2 and off2 >= 0.2, tag


def _fresh_policy(seed=5):
    from uavhip.policy import TransformerActorCritic
    torch.manual_seed(seed)
    return TransformerActorCritic().cuda()


def _golden_policy(policy_npz, tag):
    from uavhip.policy import TransformerActorCritic
    net = TransformerActorCritic()
    net.load_state_dict({k[len(f"{tag}/w/"):]: torch.from_numpy(policy_npz[k].copy()) for k in policy_npz.files
                         if k.startswith(f"{tag}/w/")})
    return net.cuda()


OFFSET_FWD = 2 ** 32 - 20
OFFSET_DEV = 12345


def _forward_draws(net, x, seed, ring, offset_dev):
    """One sampling fused_forward over windows x -> (counters, actions, p0 from the returned logits)."""
    from uavhip.policy import rowproj_buffer
    B = x.shape[0]
    lg = torch.empty(B, 2, device="cuda")
    dev = None if offset_dev is None else torch.tensor([offset_dev], dtype=torch.int64, device="cuda")
    kw = dict(rowproj=rowproj_buffer(B), step=0, fill=True) if ring else {}
    act, _, _, _, lg = net.fused_forward(x, logits=lg, seed=seed, offset=OFFSET_FWD, offset_dev=dev, **kw)
    torch.cuda.synchronize()
    counters = [OFFSET_FWD + (offset_dev or 0) + b for b in range(B)]
    return counters, act.cpu().numpy(), _p0_of_logits(lg.cpu().numpy())


@pytest.mark.parametrize("ring", [False, True], ids=["full_window", "ring"])
def test_fused_forward_draws(ring):
    """uavhip_policy_forward / _forward_rows at B = 1, 7, 37, 300 (batch tails, several workgroups),
    offset = 2^32 - 20 (the carry into the second counter word inside the batches of 37 and 300), each
    once more with offset_dev = 12345 added on the device; a key with a high word. The four batch
    sizes are one case (a batch of one draw has no power of its own); a fresh policy, p0 near 0.5.
    Measured on an MI355X, full window and ring alike: 345 decided, 0 undecided, 0 wrong per case; every
    p0 in [0.2, 0.8]; the controls disagree on 0.504 / 0.475 (counter + 1 / seed high word cleared) without
    offset_dev and 0.522 / 0.559 with it."""
    net = _fresh_policy()
    g = torch.Generator().manual_seed(17)
    for offset_dev in (None, OFFSET_DEV):
        c_all, a_all, p_all = [], [], []
        for B in (1, 7, 37, 300):
            x = torch.randn(B, 5, 14, generator=g).cuda()
            x[: B // 3, :2] = 0.0  # padded windows, as after an episode end
            c, a, p = _forward_draws(net, x, SEED_HI, ring, offset_dev)
            c_all += c
            a_all.append(a)
            p_all.append(p)
        # the batches start at the same offset: their counters repeat across (not within) batches
        _check_draws(f"fused_forward ring={ring} offset_dev={offset_dev}", SEED_HI, c_all, np.concatenate(a_all),
                     np.concatenate(p_all), unique=False)


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("ring", [False, True], ids=["full_window", "ring"])
def test_fused_forward_draws_golden_policies(policy_npz, tag, ring):
    """The golden policies of policy.npz on its 256 states: a sits at p0 = 0.5 +- 0.01, b is lopsided
    (p0 from 0.10 to 0.66). Measured on an MI355X, full window and ring alike: 256 decided, 0 undecided,
    0 wrong per case; share of p0 in [0.2, 0.8] 1.000 (a) and 0.254 (b); the controls disagree on 0.508 / 0.492
    and 0.527 / 0.562 (a, without and with offset_dev), 0.316 / 0.281 and 0.277 / 0.281 (b)."""
    net = _golden_policy(policy_npz, tag)
    x = torch.from_numpy(policy_npz["states"]).cuda()
    for offset_dev in (None, OFFSET_DEV):
        c, a, p = _forward_draws(net, x, SEED_HI, ring, offset_dev)
        _check_draws(f"golden {tag} ring={ring} offset_dev={offset_dev}", SEED_HI, c, a, p)


E_R, N_R, M_R, T_R = 37, 4, 4, 6
STRIDE = E_R + 3
OFFSET_ROLL = 2 ** 32 - 50
OFFSET_DEV_ROLL = 7


def _rollout_env(**kw):
    v = _env(N_R, M_R, 1, 1, E_R, seed=9, **kw)
    v.generate_scenes()
    return v


@pytest.mark.parametrize("entry", ["rollout_step", "rollout_steps", "rollout_actor_steps"])
def test_rollout_entry_point_draws(entry):
    """uavhip_rollout_step (T launches), _rollout_steps and _rollout_actor_steps (one launch) called
    directly: E = 37 (a partial last workgroup, one env without a partner), N = M = 4, T = 6,
    offset = 2^32 - 50, offset_stride = E + 3, offset_dev = 7: draw (t, e) uses
    offset + t * stride + *offset_dev + e, and the carry happens at t = 1.
    Measured on an MI355X, the three entry points alike: 222 decided, 0 undecided, 0 wrong; every p0 in
    [0.2, 0.8]; the controls disagree on 0.523 / 0.514."""
    from uavhip.policy import rowproj_buffer
    net = _fresh_policy()
    net.packed_weights()
    v = _rollout_env()
    E, T = E_R, T_R
    obs = torch.zeros(T + 1, E, 5, 14, device="cuda")
    v.reset(episode=1, obs_out=obs[0])
    act = torch.zeros(T, E, dtype=torch.int8, device="cuda")
    logp, val = torch.zeros(T, E, device="cuda"), torch.zeros(T, E, device="cuda")
    rew = torch.zeros(T, E, dtype=torch.float64, device="cuda")
    done = torch.zeros(T, E, dtype=torch.uint8, device="cuda")
    dev = torch.tensor([OFFSET_DEV_ROLL], dtype=torch.int64, device="cuda")
    ring = rowproj_buffer(E)
    if entry == "rollout_step":
        for t in range(T):
            net.rollout_step(v, obs[t], ring, t, t == 0, act[t], logp[t], val[t], obs[t + 1], rew[t], done[t],
                             seed=SEED_HI, offset=OFFSET_ROLL + t * STRIDE, offset_dev=dev)
    elif entry == "rollout_steps":
        net.rollout_steps(v, obs, ring, 0, True, act, logp, val, rew, done, seed=SEED_HI, offset=OFFSET_ROLL,
                          offset_stride=STRIDE, offset_dev=dev)
    else:
        net.rollout_actor_steps(v, obs, ring, 0, True, act, logp, rew, done, seed=SEED_HI, offset=OFFSET_ROLL,
                                offset_stride=STRIDE, offset_dev=dev)
    torch.cuda.synchronize()
    assert int(v.errors().abs().max()) == 0
    counters = [[OFFSET_ROLL + t * STRIDE + OFFSET_DEV_ROLL + e for e in range(E)] for t in range(T)]
    a = act.cpu().numpy()
    _check_draws(entry, SEED_HI, counters, a, _p0_of_logp(a, logp.cpu().numpy()))


ENGINE_PATHS = {
    "deferred_value": {},
    "deferred_value_graph": {},
    "persistent": dict(persistent=True),
    "fused_step": dict(fused_step=True, persistent=False),
    "forward_then_env_step": dict(fused_step=False),
}


@pytest.mark.parametrize("path", list(ENGINE_PATHS))
@pytest.mark.parametrize("setup", ["env_base", "counter_preset"])
def test_rollout_engine_draws(path, setup):
    """RolloutEngine, E = 37, N = M = 4, T = 6, at least three iterations of each launch path (the
    default one eagerly and as a captured graph, whose warm-up iteration counts as the first): draw
    (i, t, e) uses preset + i * (T + 1) * total + t * total + env_base + e -- once with env_base = 100
    of total_envs = 300, once with the device counter preset to 2^32 - 50. No counter occurs twice.
    Measured on an MI355X: 666 draws per case (888 through the graph), 0 undecided, 0 wrong; every p0 in
    [0.2, 0.8]; the controls disagree on 0.479 / 0.464 (env_base; graph 0.486 / 0.467) and 0.518 / 0.515
    (counter preset; graph 0.497 / 0.526)."""
    from uavhip.rollout import RolloutEngine
    net = _fresh_policy()
    E, T = E_R, T_R
    if setup == "env_base":
        v, total, base, preset = _rollout_env(env_base=100), 300, 100, 0
        eng = RolloutEngine(v, net, T, seed=SEED_HI, total_envs=300, **ENGINE_PATHS[path])
    else:
        v, total, base, preset = _rollout_env(), E, 0, 2 ** 32 - 50
        eng = RolloutEngine(v, net, T, seed=SEED_HI, **ENGINE_PATHS[path])
        eng.counter.fill_(preset)
    assert eng.total == total and eng.env_base == base
    assert eng.deferred_value == path.startswith("deferred_value")
    eng.start(generate=False)
    counters, actions, p0 = [], [], []

    def take(i):
        torch.cuda.synchronize()
        tr = eng.traj
        a = tr.actions.cpu().numpy().copy()
        counters.append([[preset + i * (T + 1) * total + t * total + base + e for e in range(E)] for t in range(T)])
        actions.append(a)
        p0.append(_p0_of_logp(a, tr.logp.cpu().numpy()))

    first = 0
    if path.endswith("graph"):
        eng.capture()  # its warm-up run outside the capture is iteration 0
        take(0)
        first = 1
    for i in range(first, first + 3):
        eng.collect()
        take(i)
    assert int(eng.counter.item()) == preset + (first + 3) * (T + 1) * total
    assert int(v.errors().abs().max()) == 0
    _check_draws(f"engine {path} {setup}", SEED_HI, counters, actions, p0)
