"""Host restatement of the two on-device random decisions that feed training, in numpy integers and
float64: the action-sampling draw (include/uavhip.h, "Sampling counter" at uavhip_policy_forward) and
the scene generator (include/uavhip.h, "Scene counters" at uavhip_scene_generate; the device code is
gen_scene_wave, csrc/env_device.hpp). tests/test_device_rng_host.py checks this file against the
Random123 known answers and the reference's distribution on the CPU; tests/test_gpu_device_rng.py
compares the kernels with it draw by draw and scene by scene."""
import numpy as np

_U = np.uint64
M32 = _U(0xFFFFFFFF)
_S32, _S11, _S8 = _U(32), _U(11), _U(8)
_MUL0, _MUL1 = _U(0xD2511F53), _U(0xCD9E8D57)
_W0, _W1 = _U(0x9E3779B9), _U(0xBB67AE85)
SAMPLE_C2, SAMPLE_C3 = 0x5EED, 0x9E37  # the sampling draw's third and fourth counter words

FIELDS = ("uav_type", "uav_pos", "uav_vel", "uav_load", "uav_cost", "tgt_id", "tgt_value", "tgt_pos", "tgt_vel",
          "nfz_pos", "icp_pos", "icp_vel")

# (N, M, Kn, Ki, E) of the scene comparisons, host and GPU
SCENE_SHAPES = (
    (1, 1, 0, 0, 5),      # n_remain = 0, no type-2 UAV, no obstacle arrays read
    (3, 3, 1, 1, 5),      # n_remain = 1
    (4, 4, 1, 1, 9),      # the fixture size, a partial last workgroup
    (16, 32, 2, 3, 6),    # the main size with several obstacles
    (64, 64, 8, 8, 3),    # a full wave, UAVHIP_MAX_OBSTACLES
    (5, 65, 1, 1, 3),     # the first target on a lane's second slot
    (64, 128, 1, 1, 2),   # both slots full
)


def _w(x):
    """The low 32 bits of Python ints / integer arrays, as uint64 (Python ints may exceed 2^63)."""
    if isinstance(x, (int, np.integer)):
        return _U(int(x) & 0xFFFFFFFF)
    return np.asarray(x).astype(np.uint64) & M32


def philox_v(counter4, k0, k1):
    """Philox4x32-10 (Salmon et al., Random123) on arrays: four counter words and two key words, each
    an integer or an integer array (broadcast together, the low 32 bits used) -> four uint64 arrays of
    32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(_w(x) for x in counter4))
    k0, k1 = _w(k0), _w(k1)
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return c0, c1, c2, c3


def u01(a, b):
    """The 53-bit uniform in [0, 1) of two words: the top 53 bits of (a << 32) | b, times 2^-53."""
    v = ((_w(a) << _S32) | _w(b)) >> _S11
    return v.astype(np.float64) * 2.0 ** -53


def u01f(a):
    """The 24-bit uniform in [0, 1) of one word, (a >> 8) * 2^-24: the value the kernel holds in fp32."""
    return (_w(a) >> _S8).astype(np.float64) * 2.0 ** -24


def sample_uniform(seed, c):
    """The uniform the policy kernels compare with p0 for the 64-bit sampling counter(s) c (Python
    ints or an integer array, taken modulo 2^64): the first word of philox((c_lo, c_hi, 0x5eed, 0x9e37),
    (seed_lo, seed_hi)) through u01f. The action is 0 iff u < p0."""
    c = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in np.ravel(c)], dtype=np.uint64).reshape(np.shape(c))
    seed = int(seed)
    r = philox_v((c & M32, c >> _S32, SAMPLE_C2, SAMPLE_C3), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return u01f(r[0])


def _rank(key, n):
    """Rank of key[i] among key[:n], ties broken by index (rank_in_wave): a permutation of 0..n-1."""
    k = key[:n]
    i = np.arange(n)
    less = (k[None, :] < k[:, None]) | ((k[None, :] == k[:, None]) & (i[None, :] < i[:, None]))
    return less.sum(1)


def _cos_sin(ang):
    """cos and sin evaluated in np.longdouble and rounded once to double."""
    x = np.asarray(ang, np.float64).astype(np.longdouble)
    return np.cos(x).astype(np.float64), np.sin(x).astype(np.float64)


def scene_np(seed, env_index, gen, N, M, Kn, Ki, gen_params):
    """Scene number `gen` of global env `env_index` (env_base + e) under Philox key `seed`, stream by
    stream as gen_scene_wave draws it; gen_params is uavhip.config.gen_vector(config). Every float64
    expression is written in the kernel's operation order (the kernel compiles without contraction).
    -> a dict of FIELDS: uav_* [N, ...], tgt_* [M, ...] in list order, nfz_pos [Kn, 2], icp_* [Ki, 2]."""
    g = np.asarray(gen_params, np.float64)
    (UX0, UX1, TX0, TX1, H, WS, WL, NX0, NX1, IX0, IX1, IS0, IS1) = (np.float64(v) for v in g[:13])
    seed = int(seed)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    ue, ug = int(env_index) & 0xFFFFFFFF, int(gen) & 0xFFFFFFFF
    zero = np.float64(0.0)

    def draw(index, stream):
        return philox_v((index, ue, ug, stream), k0, k1)

    out = {}
    # streams 0-2, counter index = the UAV: type shuffle key, position, speed and heading
    lane = np.arange(N)
    rk, ru, rv = draw(lane, 0), draw(lane, 1), draw(lane, 2)
    is1 = _rank(rk[0], N) >= N // 4
    us = u01(rv[0], rv[1])
    base_speed = np.where(is1, 0.35 + (0.50 - 0.35) * us, 0.75 + (0.90 - 0.75) * us)
    speed = base_speed * WS
    deg = -15.0 + (15.0 - -15.0) * u01(rv[2], rv[3])
    cs, sn = _cos_sin(deg * (np.pi / 180.0))
    out["uav_type"] = np.where(is1, 1, 2).astype(np.int32)
    out["uav_pos"] = np.stack([UX0 + (UX1 - UX0) * u01(ru[0], ru[1]), zero + (H - zero) * u01(ru[2], ru[3])], -1)
    out["uav_vel"] = np.stack([cs * speed, sn * speed], -1)
    out["uav_load"] = np.where(is1, 0.95, 1.0) * WL
    out["uav_cost"] = np.where(is1, 1.0, 1.25)
    # stream 3, counter index 0: n2, the number of 6-valued targets
    n1 = M // 2
    n_remain = M - n1 - 1
    n2 = 0
    if n_remain >= 1:
        rn = draw(0, 3)
        n2 = min(n_remain, 1 + int(float(u01(rn[0], rn[1])) * n_remain))
    n3 = n_remain - n2
    # stream 4, counter index = the list position: word 0 the id key, word 1 the value key
    t = np.arange(M)
    r4 = draw(t, 4)
    rval = _rank(r4[1], M)
    out["tgt_id"] = _rank(r4[0], M).astype(np.int32)
    out["tgt_value"] = np.where(rval < n1, 4.0, np.where(rval < n1 + n2, 6.0, np.where(rval < n1 + n2 + n3, 8.0, 16.0)))
    # streams 5 and 6: target position and velocity
    r5, r6 = draw(t, 5), draw(t, 6)
    out["tgt_pos"] = np.stack([TX0 + (TX1 - TX0) * u01(r5[0], r5[1]), zero + (H - zero) * u01(r5[2], r5[3])], -1)
    out["tgt_vel"] = np.stack([(u01(r6[0], r6[1]) - 0.5) * 0.03, (u01(r6[2], r6[3]) - 0.5) * 0.03], -1)
    # stream 7: no-fly zones
    r7 = draw(np.arange(Kn), 7)
    out["nfz_pos"] = np.stack([NX0 + (NX1 - NX0) * u01(r7[0], r7[1]), zero + (H - zero) * u01(r7[2], r7[3])], -1)
    # streams 8 and 9: interceptor position, speed and heading
    r8, r9 = draw(np.arange(Ki), 8), draw(np.arange(Ki), 9)
    out["icp_pos"] = np.stack([IX0 + (IX1 - IX0) * u01(r8[0], r8[1]), zero + (H - zero) * u01(r8[2], r8[3])], -1)
    sp = IS0 + (IS1 - IS0) * u01(r9[0], r9[1])
    cs, sn = _cos_sin(zero + (2.0 * np.pi - zero) * u01(r9[2], r9[3]))
    out["icp_vel"] = np.stack([cs * sp, sn * sp], -1)
    out["n2"] = n2
    return out
