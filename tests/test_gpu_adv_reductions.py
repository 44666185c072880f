"""GPU: the advantage kernels of csrc/gae.hip at the shapes their other tests leave out, plus
uavhip_episode_stats with a full record buffer. Marked gpu.

  * k_gae stages 64 steps x 64 envs per pass: ragged env blocks together with several passes, `done`
    flags on both sides of every pass boundary, bitwise against oracle.gae.gae_2d; its fp64 block
    partials against exact sums.
  * uavhip_adv_partials on its own (every slot written, empty blocks exactly 0.0).
  * uavhip_adv_normalize: the 64-lane chunks of the partials' fold, the tail loop beyond 2048 x 1024
    elements, n_total > n, constant input, a single element.

Bars. A partial pair is an fp64 sum of at most n terms in a fixed order, so it is within
n * 2^-53 * sum |term| of the exact sum (every term of the sum of squares is exact in fp64: a
product of two fp32 numbers). The statistics follow from the two totals: the mean inherits the
sum's bound; the variance (S2 - S mean) / (n - 1) has absolute error at most about 2 n 2^-53 S2 /
(n - 1), so with q = S2 / ((n - 1) var) the standard deviation is within q (n + 8) 2^-53 relative --
half the variance's, doubled for the handful of roundings after the sums. The inputs keep the mean
at 0.3 standard deviations (q = 1.09), so nothing cancels. The normalised elements are compared bit
for bit with fl(fl(a - (float)mean) / fl((float)std + 1e-7f)) formed from the kernel's own stats_out:
gae.hip builds without contraction and hipcc's fp32 division is correctly rounded by default
(-fhip-fp32-correctly-rounded-divide-sqrt; k_adv_normalize's code has the v_div_scale / v_div_fmas /
v_div_fixup sequence), so there is no ulp to allow.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

U = 2.0 ** -53
NORM_GRID_ELEMS = 2048 * 1024  # uavhip_adv_normalize: at most 2048 blocks x 256 threads x 4 items


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _lib():
    from uavhip._lib import LIB, check, ptr, stream_handle
    return LIB, check, ptr, stream_handle


def _check_pair(name, got_s, got_s2, a):
    """An fp64 (sum, sum of squares) of the fp32 values a against the exact sums."""
    a = np.asarray(a, np.float64).reshape(-1)
    n = max(a.size, 1)
    s, s2 = math.fsum(a), math.fsum(a * a)
    bs, bs2 = n * U * math.fsum(np.abs(a)), n * U * s2
    assert abs(got_s - s) <= bs, (name, got_s, s, bs)
    assert abs(got_s2 - s2) <= bs2, (name, got_s2, s2, bs2)
    return abs(got_s - s) / max(bs, 1e-300), abs(got_s2 - s2) / max(bs2, 1e-300)


# ------------------------------------------------------------------ uavhip_gae
def _placed_dones(rng, T, E, shift):
    """5 % random, then by column (e + shift) % 8: a done at T-1; at 0; at the older side of every
    64-step pass boundary (t = T - 64 k); at the newer side of the next pass (t = T - 64 k - 1); at
    both; the whole column done; never done; random only."""
    d = (rng.random((T, E)) < 0.05).astype(np.uint8)
    first = np.arange(T - 64, -1, -64, dtype=np.int64)  # first step of a pass (walked last in it)
    last = first[first >= 1] - 1                        # last step of the next pass (walked first in it)
    for e in range(E):
        k = (e + shift) % 8
        if k == 0:
            d[T - 1, e] = 1
        elif k == 1:
            d[0, e] = 1
        elif k == 2:
            d[first, e] = 1
        elif k == 3:
            d[last, e] = 1
        elif k == 4:
            d[np.concatenate([first, last]), e] = 1
        elif k == 5:
            d[:, e] = 1
        elif k == 6:
            d[:, e] = 0
    return d


@pytest.mark.parametrize("boot", [False, True], ids=["no_last_value", "last_value"])
@pytest.mark.parametrize("T,E", [(65, 65), (129, 130), (128, 63), (64, 1)])
def test_gae_ragged_blocks_and_pass_boundaries(T, E, boot):
    from oracle import gae as ogae
    from uavhip.ppo import gae
    LIB = _lib()[0]
    rng = np.random.default_rng(T * 1000 + E + (500 if boot else 0))
    npart = LIB.uavhip_gae_partials(T, E)
    assert npart == -(-E // 64)
    for shift in (range(8) if E < 8 else [0]):  # a single column takes every placement in turn
        r = np.where(rng.random((T, E)) < 0.5, 0.0, rng.uniform(0, 3, (T, E)))
        d = _placed_dones(rng, T, E, shift)
        v = (rng.normal(size=(T, E)) * 3).astype(np.float32)
        lv = rng.normal(size=E).astype(np.float32) if boot else None
        out = (torch.full((T, E), float("nan"), device="cuda"), torch.full((T, E), float("nan"), device="cuda"),
               torch.full((2 * npart,), float("nan"), dtype=torch.float64, device="cuda"),
               torch.empty(2, dtype=torch.float64, device="cuda"))
        ret, adv, _ = gae(torch.from_numpy(r), torch.from_numpy(d), torch.from_numpy(v).cuda(),
                          None if lv is None else torch.from_numpy(lv).cuda(), normalize=False, out=out)
        r_o, a_o = ogae.gae_2d(r, d, v, last_values=lv)
        np.testing.assert_array_equal(_bits(ret.cpu().numpy()), _bits(r_o))
        np.testing.assert_array_equal(_bits(adv.cpu().numpy()), _bits(a_o))
        part = out[2].cpu().numpy().reshape(npart, 2)
        assert np.isfinite(part).all()
        worst = 0.0
        for b in range(npart):  # the ragged last block: its live envs only
            worst = max(worst, *_check_pair(f"block {b}", part[b, 0], part[b, 1], a_o[:, 64 * b:64 * b + 64]))
        worst = max(worst, *_check_pair("total", math.fsum(part[:, 0]), math.fsum(part[:, 1]), a_o))
        print(f"T={T} E={E} boot={boot} shift={shift}: dones {int(d.sum())}, partials at {worst:.3f} of their bound")


# ------------------------------------------------------------------ uavhip_adv_partials
@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_adv_partials_every_slot(n):
    LIB, check, ptr, stream_handle = _lib()
    rng = np.random.default_rng(n)
    a = (rng.normal(size=n) * 2 + 0.6).astype(np.float32)
    adv = torch.from_numpy(a).cuda()
    for npart in (1, 3, 64, 65, 300):
        part = torch.full((2 * npart + 2,), float("nan"), dtype=torch.float64, device="cuda")
        check(LIB.uavhip_adv_partials(ptr(adv), n, ptr(part), npart, stream_handle()), "uavhip_adv_partials")
        got = part.cpu().numpy()
        assert np.isnan(got[2 * npart:]).all()  # nothing past the last slot
        got = got[:2 * npart].reshape(npart, 2)
        assert np.isfinite(got).all()  # every slot written
        worst = 0.0
        for b in range(npart):  # block b: elements b * 256 + lane, stride npart * 256
            own = a.reshape(-1)[np.concatenate([np.arange(s, min(s + 256, n)) for s in range(b * 256, n, npart * 256)]
                                               or [np.arange(0)]).astype(np.int64)]
            if own.size == 0:
                assert got[b, 0] == 0.0 and got[b, 1] == 0.0 and not np.signbit(got[b]).any()
            worst = max(worst, *_check_pair(f"n={n} np={npart} block {b}", got[b, 0], got[b, 1], own))
        worst = max(worst, *_check_pair(f"n={n} np={npart}", math.fsum(got[:, 0]), math.fsum(got[:, 1]), a))
        print(f"n={n} np={npart}: partials at {worst:.3f} of their bound")


# ------------------------------------------------------------------ uavhip_adv_normalize
def _normalize(a, npart, n=None, n_total=0):
    """uavhip_adv_partials over all of a, then uavhip_adv_normalize of its first n elements.
    -> (the buffer afterwards, stats)."""
    LIB, check, ptr, stream_handle = _lib()
    adv = torch.from_numpy(a.copy()).cuda()
    part = torch.empty(2 * npart, dtype=torch.float64, device="cuda")
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    check(LIB.uavhip_adv_partials(ptr(adv), a.size, ptr(part), npart, stream_handle()), "uavhip_adv_partials")
    check(LIB.uavhip_adv_normalize(ptr(adv), a.size if n is None else n, ptr(part), npart, n_total, ptr(stats),
                                   stream_handle()), "uavhip_adv_normalize")
    return adv.cpu().numpy(), stats.cpu().numpy()


def _expected(a, stats):
    mean, den = np.float32(stats[0]), np.float32(stats[1]) + np.float32(1e-7)
    return (a - mean) / den


def test_normalize_grid_cap_matches_the_source():
    """The sizes below assume uavhip_adv_normalize launches ceil(n / (256 x 4)) blocks capped at 2048
    (host check: read from the source, no launch)."""
    src = open(os.path.join(PKG, "csrc", "gae.hip")).read()
    assert re.search(r"constexpr int kRedBlock = 256;", src) and re.search(r"constexpr int kNormPer = 4;", src)
    assert re.search(r"if \(blocks > 2048\) blocks = 2048;", src)
    n = NORM_GRID_ELEMS + 517
    assert -(-n // (256 * 4)) > 2048  # uncapped, this n would take 2049 blocks: the cap and the tail loop run


@pytest.mark.parametrize("n", [2, 1023, 1025, NORM_GRID_ELEMS + 517])
def test_normalize_against_fp64(n):
    rng = np.random.default_rng(n)
    a = (rng.normal(size=n) * 2 + 0.6).astype(np.float32)
    a64 = a.astype(np.float64)
    mean, std = a64.mean(), a64.std(ddof=1)
    q = math.fsum(a64 * a64) / ((n - 1) * std * std)
    mean_bar = (n + 2) * U * np.abs(a64).mean()
    std_bar = q * (n + 8) * U
    for npart in (1, 63, 64, 65, 130):
        got, stats = _normalize(a, npart)
        print(f"n={n} np={npart}: mean err {abs(stats[0] - mean):.3e} (bar {mean_bar:.3e}), "
              f"std rel err {abs(stats[1] / std - 1):.3e} (bar {std_bar:.3e})")
        assert abs(stats[0] - mean) <= mean_bar
        assert abs(stats[1] / std - 1) <= std_bar
        want = _expected(a, stats)
        head = slice(0, NORM_GRID_ELEMS)
        assert np.array_equal(_bits(got[head]), _bits(want[head]))
        if n > NORM_GRID_ELEMS:  # the tail loop's elements
            tail = slice(NORM_GRID_ELEMS, n)
            assert np.array_equal(_bits(got[tail]), _bits(want[tail]))


def test_normalize_first_shard_of_a_larger_total():
    """n < n_total (uavhip/dist.py: statistics over every rank's shard, each rank normalises its own):
    the first shard equals the same slice of the whole-buffer call bit for bit; the rest is untouched."""
    rng = np.random.default_rng(12)
    N, n = 5000, 2000
    a = (rng.normal(size=N) * 2 + 0.6).astype(np.float32)
    whole, stats_w = _normalize(a, 7)
    shard, stats_s = _normalize(a, 7, n=n, n_total=N)
    assert np.array_equal(stats_w, stats_s)
    assert np.array_equal(_bits(shard[:n]), _bits(whole[:n]))
    assert np.array_equal(_bits(shard[n:]), _bits(a[n:]))


def test_normalize_constant_input():
    a = np.full(1000, 0.75, np.float32)
    got, stats = _normalize(a, 3)
    assert stats[0] == 0.75 and stats[1] == 0.0
    assert np.array_equal(_bits(got), np.zeros(1000, np.uint32))


def test_normalize_single_element_is_nan():
    """torch's unbiased std of one element is NaN, and so is the normalised advantage."""
    got, stats = _normalize(np.array([1.5], np.float32), 1)
    assert stats[0] == 1.5 and np.isnan(stats[1]) and np.isnan(got).all()
    with pytest.warns(UserWarning, match="degrees of freedom"):
        assert torch.isnan(torch.tensor([1.5]).std())


# ------------------------------------------------------------------ uavhip_episode_stats
def test_episode_stats_with_a_full_record_buffer():
    """E = 257 (the second block has one live thread), a carry from an earlier chunk, and more finished
    episodes than max_records: n_records counts them all, exactly max_records rows are kept, each a
    distinct record of the oracle's (which ones is the atomic's business), nothing is written past the
    buffer, and the carry equals the oracle's exactly."""
    from oracle import metrics as om
    from uavhip import _lib as L
    LIB, check, ptr, stream_handle = _lib()
    rng = np.random.default_rng(13)
    T, E, max_records = 12, 257, 100

    def chunk(ep0):
        rew = rng.normal(size=(T, E))
        done = (rng.random((T, E)) < 0.2).astype(np.uint8)
        act = rng.integers(0, 2, size=(T, E)).astype(np.int8)
        val = rng.normal(size=(T, E)).astype(np.float32)
        info = rng.random((T, E, L.INFO_COUNT))
        info[..., L.INFO["NUM_ASSIGNED"]] = rng.integers(0, 5, size=(T, E))
        info[..., L.INFO["IS_VALID"]] = rng.integers(-1, 2, size=(T, E))
        ends = np.cumsum(done, axis=0) - done  # episodes finished before step t of this chunk
        info[..., L.INFO["EPISODE"]] = ep0[None, :] + ends
        return (rew, done, act, info, val), ep0 + done.sum(0)
    first, ep1 = chunk(np.ones(E))
    second, _ = chunk(ep1)
    _, acc0 = om.episode_records(*first)
    ref, acc1 = om.episode_records(*second, acc=acc0)
    assert len(ref) > 4 * max_records and acc0.any()

    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in second]
    acc = torch.from_numpy(acc0.copy()).cuda()
    records = torch.full((max_records + 8, L.EP_COUNT), float("nan"), dtype=torch.float64, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(LIB.uavhip_episode_stats(*(ptr(x) for x in dev), T, E, ptr(acc), ptr(records), max_records, ptr(count),
                                   stream_handle()), "uavhip_episode_stats")
    assert int(count.item()) == len(ref)
    rec = records.cpu().numpy()
    assert np.isnan(rec[max_records:]).all()
    kept = rec[:max_records]
    assert np.isfinite(kept).all()
    members = {r.tobytes() for r in ref}
    assert len(members) == len(ref)
    rows = {r.tobytes() for r in kept}
    assert len(rows) == max_records and rows <= members
    np.testing.assert_array_equal(acc.cpu().numpy(), acc1)
