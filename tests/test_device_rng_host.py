"""Host-side checks (no GPU) of tests/device_rng.py, the restatement tests/test_gpu_device_rng.py
compares the kernels with: its Philox against the scalar one of test_multistart_host.py and the
Random123 known answers, the two word-to-uniform rules at their edges, and scene_np -- the structure
of a scene at every shape the GPU test uses, the ranges of the reference's _generate_scene
(envs/uav_env.py:65-173), the four inputs of the counter, and its law: KS against the uniform laws the
reference draws from and chi-square on the discrete draws, at the significance of
test_gpu_scene_dist.py. The GPU test then ties the device to this restatement exactly."""
import numpy as np
import pytest
from scipy import stats

from device_rng import FIELDS, SCENE_SHAPES, philox_v, sample_uniform, scene_np, u01, u01f
from test_multistart_host import philox4x32_10

ALPHA = 1e-4  # per statistic, as tests/test_gpu_scene_dist.py (seeded: a run is deterministic)
M32 = 0xFFFFFFFF


def _gen(speed=1.0, load=1.0):
    from uavhip.config import Config, gen_vector
    c = Config()
    c.WEATHER_SPEED_FACTOR, c.WEATHER_LOAD_FACTOR = speed, load
    return gen_vector(c)


def test_longdouble_is_wider_than_double():
    """scene_np rounds cos and sin once from np.longdouble: that needs more than 53 bits there."""
    assert np.finfo(np.longdouble).nmant >= 63


def test_philox_v_is_the_scalar_philox():
    rng = np.random.default_rng(11)
    n = 300
    ctr = rng.integers(0, 1 << 32, (4, n), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (2, n), dtype=np.uint64)
    ctr[:, 0], key[:, 0] = 0, 0
    ctr[:, 1], key[:, 1] = M32, M32
    got = np.stack(philox_v(tuple(ctr), key[0], key[1]), 1)
    want = np.array([philox4x32_10(ctr[:, i], key[:, i]) for i in range(n)], dtype=np.uint64)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    # scalars and broadcasting: one key for every counter, Python ints beyond 32 bits use the low word
    one = philox_v((ctr[0], 5, (7 << 32) | 6, 9), (1 << 32) | 3, 4)
    assert np.array_equal(np.stack(one, 1), np.array([philox4x32_10((c, 5, 6, 9), (3, 4)) for c in ctr[0]], np.uint64))


def test_philox_v_known_answers():
    """The known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10)."""
    hexs = lambda x: " ".join(f"{int(w):08x}" for w in x)  # noqa: E731
    assert hexs(philox_v((0, 0, 0, 0), 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexs(philox_v((M32,) * 4, M32, M32)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexs(philox_v((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), 0xa4093822, 0x299f31d0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_word_to_uniform_rules():
    assert u01(0, 0) == 0.0 and u01f(0) == 0.0
    assert u01(M32, M32) == 1.0 - 2.0 ** -53 and u01f(M32) == 1.0 - 2.0 ** -24
    # one-bit steps land where the shifts say: u01 drops b's low 11 bits, u01f a's low 8
    assert u01(0, 1 << 10) == 0.0 and u01(0, 1 << 11) == 2.0 ** -53 and u01(1, 0) == 2.0 ** -32
    assert u01(1 << 31, 0) == 0.5 and u01(0, 1 << 31) == 2.0 ** -33
    assert u01f(1 << 7) == 0.0 and u01f(1 << 8) == 2.0 ** -24 and u01f(1 << 31) == 0.5
    a = np.array([0, 255, 256, M32], np.uint64)
    assert np.array_equal(u01f(a), [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24])
    assert np.array_equal(u01f(a).astype(np.float32).astype(np.float64), u01f(a))  # exact in fp32


def test_sample_uniform_counter_words():
    """The 64-bit counter splits into words 0 and 1; words 2 and 3 are 0x5eed and 0x9e37; the seed's
    halves are the key; counters wrap modulo 2^64."""
    seed = (0xDEADBEEF << 32) | 7
    c = [0, 1, (1 << 32) - 1, 1 << 32, (5 << 32) | 9, (1 << 64) - 1, (1 << 64) + 1]
    got = sample_uniform(seed, c)
    for ci, u in zip(c, got):
        ci &= (1 << 64) - 1
        w = philox4x32_10((ci & M32, ci >> 32, 0x5EED, 0x9E37), (7, 0xDEADBEEF))[0]
        assert u == (w >> 8) * 2.0 ** -24
    assert got[1] == got[6] and len(set(got[:6])) == 6
    assert sample_uniform(seed, 1 << 32) != sample_uniform(seed, 0)        # the high counter word counts
    assert sample_uniform(seed, 3) != sample_uniform(seed & M32, 3)        # and so does the seed's
    assert sample_uniform(seed, np.arange(6).reshape(2, 3)).shape == (2, 3)


def _check_structure(s, N, M, Kn, Ki, g):
    n1, n_remain = M // 2, M - M // 2 - 1
    assert sorted(s["tgt_id"]) == list(range(M))
    n2 = int((s["tgt_value"] == 6).sum())
    assert n2 == s["n2"] and (1 <= n2 <= n_remain if n_remain >= 1 else n2 == 0)
    counts = {v: int((s["tgt_value"] == v).sum()) for v in (4.0, 6.0, 8.0, 16.0)}
    assert counts == {4.0: n1, 6.0: n2, 8.0: n_remain - n2, 16.0: 1} and sum(counts.values()) == M
    assert int((s["uav_type"] == 2).sum()) == N // 4 and set(np.unique(s["uav_type"])) <= {1, 2}
    t1 = s["uav_type"] == 1
    ws, wl = g[5], g[6]
    assert np.array_equal(s["uav_cost"], np.where(t1, 1.0, 1.25))
    assert np.array_equal(s["uav_load"], np.where(t1, 0.95, 1.0) * wl)
    shapes = dict(uav_type=(N,), uav_pos=(N, 2), uav_vel=(N, 2), uav_load=(N,), uav_cost=(N,), tgt_id=(M,),
                  tgt_value=(M,), tgt_pos=(M, 2), tgt_vel=(M, 2), nfz_pos=(Kn, 2), icp_pos=(Ki, 2), icp_vel=(Ki, 2))
    assert {k: s[k].shape for k in FIELDS} == shapes
    assert s["tgt_id"].dtype == np.int32 and s["uav_type"].dtype == np.int32
    assert all(s[k].dtype == np.float64 for k in FIELDS if k not in ("tgt_id", "uav_type"))

    def inside(x, lo, hi):
        return bool(((x >= lo) & (x < hi)).all())
    eps = 1e-12  # speeds and headings are recovered through a norm / an arctan2
    assert inside(s["uav_pos"][:, 0], g[0], g[1]) and inside(s["uav_pos"][:, 1], 0.0, g[4])
    sp = np.linalg.norm(s["uav_vel"], axis=-1)
    assert inside(sp[t1], 0.35 * ws - eps, 0.50 * ws + eps) and inside(sp[~t1], 0.75 * ws - eps, 0.90 * ws + eps)
    assert inside(np.degrees(np.arctan2(s["uav_vel"][:, 1], s["uav_vel"][:, 0])), -15.0 - eps, 15.0 + eps)
    assert inside(s["tgt_pos"][:, 0], g[2], g[3]) and inside(s["tgt_pos"][:, 1], 0.0, g[4])
    assert inside(s["tgt_vel"], -0.015, 0.015)
    assert inside(s["nfz_pos"][:, 0], g[7], g[8]) and inside(s["nfz_pos"][:, 1], 0.0, g[4])
    assert inside(s["icp_pos"][:, 0], g[9], g[10]) and inside(s["icp_pos"][:, 1], 0.0, g[4])
    assert inside(np.linalg.norm(s["icp_vel"], axis=-1), g[11] - eps, g[12] + eps)


@pytest.mark.parametrize("N,M,Kn,Ki,E", SCENE_SHAPES)
def test_scene_structure_and_ranges(N, M, Kn, Ki, E):
    """Ids a permutation, the value multiset {4 x M//2, 6 x n2, 8 x n3, 16 x 1}, N//4 type-2 UAVs, every
    field inside the reference's range -- with the weather factors at 1 and away from it."""
    for g in (_gen(), _gen(0.8, 0.9)):
        for e in range(E):
            for gen in (0, 3):
                _check_structure(scene_np(77, e, gen, N, M, Kn, Ki, g), N, M, Kn, Ki, g)


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in FIELDS if a[k].size)


@pytest.mark.parametrize("N,M,Kn,Ki,E", SCENE_SHAPES)
def test_each_counter_input_matters(N, M, Kn, Ki, E):
    """Scenes differ when any one of seed low word, seed high word, env index or gen changes -- in
    every drawn field (a field that ignored one of them would repeat)."""
    g = _gen()
    seed, e, gen = (0xDEADBEEF << 32) | 7, 5, 2
    base = scene_np(seed, e, gen, N, M, Kn, Ki, g)
    assert not _differs(base, scene_np(seed, e, gen, N, M, Kn, Ki, g))
    for other in ((seed ^ 1, e, gen), (seed ^ (1 << 32), e, gen), (seed, e + 1, gen), (seed, e, gen + 1)):
        s = scene_np(*other, N, M, Kn, Ki, g)
        assert _differs(base, s), other
        for k in ("uav_pos", "uav_vel", "tgt_pos", "tgt_vel", "nfz_pos", "icp_pos", "icp_vel"):
            assert base[k].size == 0 or not np.array_equal(base[k], s[k]), (other, k)
    # env indices alias modulo 2^32, as the kernel's counter word does
    assert not _differs(base, scene_np(seed, e + (1 << 32), gen, N, M, Kn, Ki, g))


def _ks(name, x, lo, hi):
    p = stats.kstest(np.ravel(x), stats.uniform(lo, hi - lo).cdf).pvalue
    print(f"{name}: KS p = {p:.3g}")
    assert p > ALPHA, name


def _chi2(name, counts):
    p = stats.chisquare(np.asarray(counts, float)).pvalue
    print(f"{name}: chi2 p = {p:.3g} (counts {list(counts)})")
    assert p > ALPHA, name


def test_law_of_the_restatement():
    """3,000 restated 4 x 4 scenes (N//4 = 1 type-2 UAV) against the laws the reference draws from.
    At M = 4 n_remain is 1 and n2 is always 1, so the chi-square on n2 ~ U{1..n_remain} runs on 1,500
    scenes of 1 x 8 (n_remain = 3)."""
    g = _gen()
    sc = [scene_np(2024, e, e % 3, 4, 4, 1, 1, g) for e in range(3000)]
    S = {k: np.stack([s[k] for s in sc]) for k in FIELDS}
    assert all(s["n2"] == 1 for s in sc)
    t1 = S["uav_type"] == 1
    sp = np.linalg.norm(S["uav_vel"], axis=-1)
    _ks("UAV x", S["uav_pos"][..., 0], 60, 90)
    _ks("UAV y", S["uav_pos"][..., 1], 0, 160)
    _ks("type-1 speed", sp[t1], 0.35, 0.50)
    _ks("type-2 speed", sp[~t1], 0.75, 0.90)
    _ks("heading (deg)", np.degrees(np.arctan2(S["uav_vel"][..., 1], S["uav_vel"][..., 0])), -15, 15)
    _ks("target x", S["tgt_pos"][..., 0], 160, 180)
    _ks("target y", S["tgt_pos"][..., 1], 0, 160)
    _ks("target vx", S["tgt_vel"][..., 0], -0.015, 0.015)
    _ks("target vy", S["tgt_vel"][..., 1], -0.015, 0.015)
    _ks("NFZ x", S["nfz_pos"][..., 0], 120, 140)
    _ks("NFZ y", S["nfz_pos"][..., 1], 0, 160)
    _ks("interceptor x", S["icp_pos"][..., 0], 140, 160)
    _ks("interceptor y", S["icp_pos"][..., 1], 0, 160)
    _ks("interceptor speed", np.linalg.norm(S["icp_vel"], axis=-1), 0.30, 0.32)
    _ks("interceptor heading", np.mod(np.arctan2(S["icp_vel"][..., 1], S["icp_vel"][..., 0]), 2 * np.pi), 0, 2 * np.pi)
    _chi2("position of the 16-value target", np.bincount(np.argmax(S["tgt_value"] == 16, 1), minlength=4))
    _chi2("position of id 0", np.bincount(np.argmax(S["tgt_id"] == 0, 1), minlength=4))
    _chi2("index of the type-2 UAV", np.bincount(np.argmax(S["uav_type"] == 2, 1), minlength=4))
    n2 = np.array([scene_np(2024, e, 0, 1, 8, 0, 0, g)["n2"] for e in range(1500)])
    assert n2.min() == 1 and n2.max() == 3
    _chi2("n2 ~ U{1..3}", np.bincount(n2, minlength=4)[1:])
    # two fields must not share a stream: the draws of different fields are uncorrelated
    pairs = (("uav_pos", "tgt_pos"), ("tgt_pos", "tgt_vel"), ("nfz_pos", "icp_pos"), ("uav_pos", "uav_vel"))
    for a, b in pairs:
        r = np.corrcoef(S[a][:, 0, 0], S[b][:, 0, 0])[0, 1]
        print(f"corr({a}, {b}) = {r:.3g}")
        assert abs(r) < 5 / np.sqrt(len(sc)), (a, b, r)
