"""CPU: tests/adam_model.py pinned bitwise to torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam(foreach=False) on CPU tensors, the arithmetic k_adam's contract names.

Two tensors (33 and 20 000 elements: torch's vector body and its scalar tail), one per parameter
group (2e-4 and 1e-3), 10 consecutive steps from zero moments, clip inactive and active, beta1 0.9
and 0.8. Clipped g, exp_avg, exp_avg_sq and p are compared bit for bit after every step; the model
is then set to torch's state, so one mismatch does not cascade.

Gradients are +-2^k with each tensor's sum of squares a power of four (adam_model.pow4_gradient), so
the norm is exact in any summation order and through clip_grad_norm_'s norm of norms. After an active
clip the gradients are no longer powers of two: w2 * g and v * b2 both round, which is where the
fused multiply-add in v shows.

The test bites: with the model's v unfused (v * b2 + (w2 * g) * g, every operation rounded) the
clip-active beta1 = 0.9 run disagrees with torch in exp_avg_sq in 12 815 element-steps of 200 330
(and then in p in 13); test_unfused_v_differs_from_torch keeps that from silently becoming zero.
With the clip inactive the gradients stay powers of two and both forms agree, as they should.

One operation of torch's is not an IEEE operation: Tensor.sqrt on a CPU tensor (torch 2.10 with MKL's
vector maths) returns a value one ulp below the correctly rounded root for 0.5 to 1 % of inputs
(measured here: 909 to 1 883 of 200 330 element-steps per run). The kernel's sqrtf and
numpy's sqrt are correctly rounded, and the model keeps numpy's by default. So p is checked twice:
bitwise against torch with torch's own sqrt passed in as the model's root (this pins the operation
order and every other rounding of the division chain, over every element), and with the correctly
rounded root, where p may differ from torch only in elements whose torch root is itself off (0 to 6
element-steps per run; none anywhere else). torch's root is asserted to be within one ulp.
"""
import numpy as np
import pytest
import torch

import adam_model as am

SIZES = (33, 20000)
LRS = (2e-4, 1e-3)
STEPS = 10


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _torch_sqrt(v):
    """torch's own CPU sqrt, tensor by tensor as the optimizer calls it."""
    parts = np.split(np.ascontiguousarray(v, dtype=np.float32), np.cumsum(SIZES)[:-1])
    return np.concatenate([torch.from_numpy(x.copy()).sqrt().numpy() for x in parts])


def _run(clip, beta1, fused_v=True, seed=0):
    """-> mismatching element-steps per compared quantity, plus the largest and smallest coefficient."""
    rng = np.random.default_rng(seed)
    params = [torch.nn.Parameter(torch.from_numpy(rng.normal(size=n).astype(np.float32))) for n in SIZES]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, LRS)], betas=(beta1, 0.999),
                           eps=1e-8, foreach=False)
    lr = np.concatenate([np.full(n, l) for n, l in zip(SIZES, LRS)])
    m = np.zeros(sum(SIZES), np.float32)
    v = np.zeros(sum(SIZES), np.float32)
    bad = dict(g=0, m=0, v=0, p=0, p_ieee_sqrt=0, sqrt_off=0, p_unexplained=0)
    coefs = []
    for t in range(1, STEPS + 1):
        # sum of squares 4^a + 4^b: below 1 (inactive) or between 5 and 80 (active), varying by step
        js = rng.integers(-3, 0, size=2) if not clip else rng.integers(1, 4, size=2)
        gs = [am.pow4_gradient(rng, n, int(j)) for n, j in zip(SIZES, js)]
        p0 = np.concatenate([p.detach().numpy().copy() for p in params])
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        g_t = np.concatenate([p.grad.numpy().copy() for p in params])
        opt.step()
        g_m, m_m, v_m, p_m, coef = am.clip_adam_step(p0, np.concatenate(gs), m, v, t, lr, beta1=beta1,
                                                     fused_v=fused_v, sqrt=_torch_sqrt)
        p_i = am.clip_adam_step(p0, np.concatenate(gs), m, v, t, lr, beta1=beta1, fused_v=fused_v)[3]
        coefs.append(float(coef))
        m_t = np.concatenate([opt.state[p]["exp_avg"].numpy() for p in params])
        v_t = np.concatenate([opt.state[p]["exp_avg_sq"].numpy() for p in params])
        p_t = np.concatenate([p.detach().numpy() for p in params])
        for k, a, b in (("g", g_m, g_t), ("m", m_m, m_t), ("v", v_m, v_t), ("p", p_m, p_t)):
            bad[k] += int(np.count_nonzero(_bits(a) != _bits(b)))
        # torch's sqrt against the correctly rounded one: never more than one ulp apart, and the only
        # reason the model with the correctly rounded sqrt may differ from torch in p
        off = _bits(_torch_sqrt(v_m)) != _bits(np.sqrt(v_m))
        assert np.abs(_bits(_torch_sqrt(v_m)).astype(np.int64) - _bits(np.sqrt(v_m)).astype(np.int64)).max() <= 1
        p_off = _bits(p_i) != _bits(p_t)
        bad["sqrt_off"] += int(off.sum())
        bad["p_ieee_sqrt"] += int(p_off.sum())
        bad["p_unexplained"] += int((p_off & ~off).sum())
        assert int(opt.state[params[0]]["step"]) == t
        m, v = m_t.copy(), v_t.copy()  # the next step starts from torch's state
    return bad, min(coefs), max(coefs)


@pytest.mark.parametrize("beta1", [0.9, 0.8])
@pytest.mark.parametrize("clip", [False, True], ids=["clip_inactive", "clip_active"])
def test_model_is_bitwise_torch_cpu(clip, beta1):
    bad, cmin, cmax = _run(clip, beta1)
    print(f"clip={clip} beta1={beta1}: mismatching element-steps {bad}, coef in [{cmin:.6g}, {cmax:.6g}]")
    if clip:
        assert cmax < 0.5
    else:
        assert cmin == cmax == 1.0
    assert (bad["g"], bad["m"], bad["v"], bad["p"]) == (0, 0, 0, 0)
    assert bad["p_unexplained"] == 0  # with the correctly rounded sqrt: off only where torch's sqrt is


def test_unfused_v_differs_from_torch():
    """The unfused v is one ulp off torch's in a few percent of elements once the clipped gradients
    are no longer powers of two; everything computed before v still agrees."""
    bad, _, _ = _run(True, 0.9, fused_v=False)
    print(f"unfused v: mismatching element-steps {bad} of {STEPS * sum(SIZES)}")
    assert bad["g"] == 0 and bad["m"] == 0
    assert bad["v"] > 0


def test_fma32_breaks_double_rounding_ties():
    """a * b + c whose fp64 sum lands exactly on an fp32 tie while the exact value lies just off it:
    rounding the fp64 sum to fp32 (ties to even) goes the wrong way; the residual decides."""
    ulp = np.float32(2.0 ** -23)
    tiny = np.float32(2.0 ** -80)
    a = np.float32(1.0 + 2.0 ** -12)  # a * a = 1 + 2^-11 + 2^-24: halfway between two fp32 numbers
    lo = np.float32(1.0 + 2.0 ** -11)  # the even one of the two
    assert am.fma32(a, a, np.float32(0.0)) == lo  # a true tie: to even
    # the fp64 sum is the tie itself (2^-80 is far below its last bit); only the residual tells
    assert am.fma32(a, a, tiny) == lo + ulp
    assert am.fma32(a, a, -tiny) == lo
    assert np.float32(np.float64(a) * np.float64(a) + np.float64(tiny)) == lo  # what plain fp64 would give
    # and against exact rational arithmetic on random operands
    from fractions import Fraction
    rng = np.random.default_rng(3)
    x, y, z = (rng.normal(size=2000).astype(np.float32) for _ in range(3))
    z *= np.float32(2.0) ** rng.integers(-30, 30, size=2000).astype(np.float32)
    got = am.fma32(x, y, z)
    for i in range(2000):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo = np.nextafter(got[i], np.float32(-np.inf))
        hi = np.nextafter(got[i], np.float32(np.inf))
        d = abs(Fraction(float(got[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), i
