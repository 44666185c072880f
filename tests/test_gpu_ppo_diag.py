"""uavhip_ppo_diagnostics (csrc/ppo_diag.hip) against a numpy fp64 restatement summed with math.fsum.

The device computes every per-sample term with the same IEEE double operations as the restatement
(fp contraction is off), except exp, whose last bit may differ between the device's and numpy's
library. So a sum differs from the exactly rounded one by its summation order and by the exp:

  sums        |S_dev - S_ref| <= n 2^-53 sum|term|   (n - 1 additions, each within 2^-53 of its partial
                                                       sum, every partial sum <= sum|term|; first order)
              + 2^-51 sum r_i                         where an exp enters (one ulp each side: 2 x 2^-52 r_i)
  means       the sum's bar divided by n
  variances   64 n 2^-53 relative (Welford / pairwise merges: a few roundings per sample on
              quantities bounded by the variance's own terms; 64 covers the constant)
  RATIO_MAX   2^-51 relative (the two exps)
  fractions, NONFINITE: exact, given that no |r_i - 1| and no |dv_i| lies within 1e-9 of eps_clip (a
              last-ulp exp difference is ~1e-16: it cannot flip a comparison); asserted on the inputs
  EXPLAINED_VAR = 1 - Var(x) / Var(y): both variances within their bar v = 64 n 2^-53 relative, the
              division and the subtraction one rounding each: |d EV| <= (Var x / Var y) (2 v + 2^-52) + 2^-53 |EV|

Every test prints the errors it measures beside the bars."""
import math

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

EPS = 0.2
U = 2.0 ** -53
SIZES = (1, 63, 64, 65, 257, 8209)
_CACHE = {}


def make_inputs(n, seed=0):
    """(old_logp, new_logp, old_value, new_value, returns) float32 [n]; no ratio and no value step
    within 1e-9 of the clip threshold."""
    key = (n, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * seed + n)
        old = (-0.69 + 0.1 * rng.standard_normal(n)).astype(np.float32)
        new = (old + 0.15 * rng.standard_normal(n)).astype(np.float32)
        ov = rng.standard_normal(n).astype(np.float32)
        nv = (ov + 0.3 * rng.standard_normal(n)).astype(np.float32)
        R = (1.0 + 2.0 * rng.standard_normal(n)).astype(np.float32)
        for a in (old, new, ov, nv, R):
            a.setflags(write=False)
        _CACHE[key] = (old, new, ov, nv, R)
    return _CACHE[key]


def reference(old, new, ov, nv, R, eps=EPS):
    """The fp64 restatement: exactly rounded sums (math.fsum) of the same per-sample terms."""
    n = len(old)
    with np.errstate(all="ignore"):
        d = new.astype(np.float64) - old.astype(np.float64)
        r = np.exp(d)
        kl = (r - 1.0) - d
        dv = nv.astype(np.float64) - ov.astype(np.float64)
        x = R.astype(np.float64) - ov.astype(np.float64)
        y = R.astype(np.float64)
        fin = np.isfinite(d)
        ref = {"n": n, "kl_sum": math.fsum(kl) if fin.all() else float(np.sum(kl)),
               "kl_abs": math.fsum(np.abs(kl[fin])), "r_sum": math.fsum(r[np.isfinite(r)]),
               "clip": int(np.sum(np.abs(r - 1.0) > eps)), "vclip": int(np.sum(np.abs(dv) > eps)),
               "rmax": float(np.nanmax(r)), "nonfinite": int(np.sum(~fin)),
               "margin": float(min(np.min(np.abs(np.abs(r[fin] - 1.0) - eps), initial=1.0),
                                   np.min(np.abs(np.abs(dv) - eps))))}
        mx, my = math.fsum(x) / n, math.fsum(y) / n
        ref["var_x"] = math.fsum((x - mx) ** 2) / n
        ref["var_y"] = math.fsum((y - my) ** 2) / n
    return ref


def run(arrs, eps=EPS):
    from uavhip.ppo import ppo_diagnostics
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.array(a, dtype=np.float32)).to(dev) for a in arrs]  # a writable copy
    return ppo_diagnostics(t[0], t[1], t[2], t[3], t[4], eps_clip=eps)


def slots(out):
    from uavhip import _lib
    v = out.cpu().numpy()
    return {k: float(v[i]) for k, i in _lib.DIAG.items()}


@pytest.mark.parametrize("n", SIZES)
def test_random_inputs_within_the_derived_bars(n):
    arrs = make_inputs(n)
    ref = reference(*arrs)
    assert ref["margin"] > 1e-9, "an input lies within 1e-9 of the clip threshold"
    assert ref["nonfinite"] == 0
    got = slots(run(arrs))
    exp_bar = 2.0 ** -51 * ref["r_sum"]
    kl_bar = (n * U * ref["kl_abs"] + exp_bar) / n
    rm_bar = (n * U * ref["r_sum"] + exp_bar) / n
    var_bar = 64 * n * U
    e_kl = abs(got["APPROX_KL"] - ref["kl_sum"] / n)
    e_rm = abs(got["RATIO_MEAN"] - ref["r_sum"] / n)
    e_max = abs(got["RATIO_MAX"] - ref["rmax"]) / ref["rmax"]
    print(f"n={n}: |d KL| {e_kl:.3e} (bar {kl_bar:.3e}), |d ratio mean| {e_rm:.3e} (bar {rm_bar:.3e}), "
          f"ratio max rel {e_max:.3e} (bar {2.0 ** -51:.3e})")
    assert e_kl <= kl_bar and e_rm <= rm_bar and e_max <= 2.0 ** -51
    assert got["CLIP_FRAC"] == ref["clip"] / n and got["VALUE_CLIP_FRAC"] == ref["vclip"] / n
    assert got["NONFINITE"] == 0.0
    assert 0 < ref["clip"] < n or n == 1  # the inputs exercise both sides of the clamp
    if n == 1:  # one sample: both variances exactly 0, the explained variance undefined
        assert got["RETURN_VAR"] == 0.0 and got["RESIDUAL_VAR"] == 0.0 and math.isnan(got["EXPLAINED_VAR"])
        return
    e_vx = abs(got["RESIDUAL_VAR"] - ref["var_x"]) / ref["var_x"]
    e_vy = abs(got["RETURN_VAR"] - ref["var_y"]) / ref["var_y"]
    ev_ref = 1.0 - ref["var_x"] / ref["var_y"]
    ev_bar = ref["var_x"] / ref["var_y"] * (2 * var_bar + 2 * U) + U * abs(ev_ref)
    e_ev = abs(got["EXPLAINED_VAR"] - ev_ref)
    print(f"n={n}: Var(R - V) rel {e_vx:.3e}, Var(R) rel {e_vy:.3e} (bar {var_bar:.3e}), "
          f"|d EV| {e_ev:.3e} (bar {ev_bar:.3e})")
    assert e_vx <= var_bar and e_vy <= var_bar and e_ev <= ev_bar


@pytest.mark.parametrize("n", (1, 65, 8209))
def test_new_equal_to_old(n):
    old, _, ov, _, R = make_inputs(n)
    got = slots(run((old, old, ov, ov, R)))
    assert got["APPROX_KL"] == 0.0 and got["CLIP_FRAC"] == 0.0 and got["VALUE_CLIP_FRAC"] == 0.0
    assert got["RATIO_MAX"] == 1.0 and got["RATIO_MEAN"] == 1.0 and got["NONFINITE"] == 0.0


@pytest.mark.parametrize("n", (65, 8209))
def test_every_sample_clipped(n):
    old, _, ov, _, R = make_inputs(n)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    arrs = (old, old + sign, ov, ov - sign, R)  # r = e or 1 / e, |dv| = 1: every sample beyond the clamp
    ref = reference(*arrs)
    assert ref["margin"] > 1e-9 and ref["clip"] == n and ref["vclip"] == n
    got = slots(run(arrs))
    assert got["CLIP_FRAC"] == 1.0 and got["VALUE_CLIP_FRAC"] == 1.0
    bar = (n * U * ref["kl_abs"] + 2.0 ** -51 * ref["r_sum"]) / n
    err = abs(got["APPROX_KL"] - ref["kl_sum"] / n)
    print(f"n={n}: |d KL| {err:.3e} (bar {bar:.3e})")
    assert err <= bar


@pytest.mark.parametrize("n", (65, 8209))
def test_constant_returns_and_perfect_values(n):
    old, new, ov, nv, R = make_inputs(n)
    const = np.full(n, 0.1, np.float32)  # not a dyadic rational: sum(x^2) - sum(x)^2 / n would not be 0
    got = slots(run((old, new, ov, nv, const)))
    assert got["RETURN_VAR"] == 0.0 and math.isnan(got["EXPLAINED_VAR"])
    assert got["RESIDUAL_VAR"] > 0.0
    got = slots(run((old, new, R, nv, R)))  # V_old == R: nothing left to explain
    assert got["RESIDUAL_VAR"] == 0.0 and got["EXPLAINED_VAR"] == 1.0


def test_one_infinite_log_prob_is_counted_and_propagates():
    n = 8209
    old, new, ov, nv, R = make_inputs(n)
    new = new.copy()
    new[4321] = -np.inf  # d = -inf, r = 0: the KL term is +inf
    ref = reference(old, new, ov, nv, R)
    got = slots(run((old, new, ov, nv, R)))
    assert got["NONFINITE"] == 1.0 == ref["nonfinite"]
    assert got["APPROX_KL"] == math.inf  # nothing is clamped
    assert got["CLIP_FRAC"] == ref["clip"] / n and got["VALUE_CLIP_FRAC"] == ref["vclip"] / n
    assert math.isfinite(got["RATIO_MEAN"]) and math.isfinite(got["EXPLAINED_VAR"])
    nan = new.copy()
    nan[4321] = np.nan  # d = NaN: counted, in the sums, skipped by the maximum
    got = slots(run((old, nan, ov, nv, R)))
    assert got["NONFINITE"] == 1.0 and math.isnan(got["APPROX_KL"]) and math.isnan(got["RATIO_MEAN"])
    assert abs(got["RATIO_MAX"] - ref["rmax"]) <= 2.0 ** -51 * ref["rmax"]


@pytest.mark.parametrize("n", (257, 8209))
def test_two_identical_calls_are_bitwise_equal(n):
    arrs = make_inputs(n, seed=1)
    a, b = run(arrs), run(arrs)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_update_diagnostics_runs_the_forward_over_the_batch():
    """uavhip.ppo.update_diagnostics: the fused forward's log-probabilities and values of the batch
    into the kernel. Against a policy that has not changed since the batch was recorded the ratio is
    exactly 1; `out` and the dict form agree; the policy's sampling counter is left alone."""
    from uavhip import _lib
    from uavhip.policy import TransformerActorCritic
    from uavhip.ppo import update_diagnostics
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = TransformerActorCritic().to(dev)
    n = 321
    x = torch.randn(n, 5, 14, device=dev)
    a = torch.randint(0, 2, (n,), device=dev).to(torch.int8)
    _, lp, v, _, _ = net.fused_forward(x, actions=a, offset=0)
    R = torch.randn(n, device=dev)
    before = net._sample_offset
    d = update_diagnostics(net, x, a, lp, v, R)
    assert net._sample_offset == before
    assert set(d) == {k.lower() for k in _lib.DIAG}
    assert float(d["approx_kl"]) == 0.0 and float(d["ratio_max"]) == 1.0 and float(d["clip_frac"]) == 0.0
    assert float(d["value_clip_frac"]) == 0.0 and float(d["nonfinite"]) == 0.0
    out = torch.zeros(_lib.DIAG_COUNT, dtype=torch.float64, device=dev)
    assert update_diagnostics(net, x, a, lp, v, R, out=out) is out
    assert all(float(out[i]) == float(d[k.lower()]) or math.isnan(float(out[i])) for k, i in _lib.DIAG.items())
    # shifted old log-probabilities: r = exp(0.25) for every sample
    d = update_diagnostics(net, x, a, lp - 0.25, v, R)
    assert abs(float(d["ratio_mean"]) - math.exp(0.25)) < 1e-6 and float(d["clip_frac"]) == 1.0
