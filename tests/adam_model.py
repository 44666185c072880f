"""Test infrastructure: one `clip_grad_norm_` + single-tensor Adam step restated in numpy, every
operation rounded to fp32 exactly where torch's CPU path (torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam(foreach=False) on CPU tensors) rounds. This is the arithmetic k_adam
(csrc/train.hip) documents as its contract; tests/test_adam_model_host.py pins the model bitwise to
torch on the CPU and tests/test_gpu_adam_update.py pins the kernel bitwise to the model.

    norm  = fp32 sqrt of the fp32 sum of squares
    coef  = min(max_norm / (norm + 1e-6f), 1)
    g     = g * coef
    m     = fma(w1, g - m, m)                  w1 = (float)(1 - b1)
    v     = fma(w2 * g, g, v * b2)             w2 = (float)(1 - b2), b2 = (float)b2
    denom = sqrt(v) / bc2s + eps
    p     = p + (nss * m) / denom
    nss   = (float)(-(lr / (1 - b1^t)))        formed in double, as adam_advance does
    bc2s  = (float)sqrt(1 - b2^t)              formed in double

Limits of the restatement (said here, not tested):
  * beta1 < 0.5 makes the lerp weight 1 - b1 >= 0.5, where torch takes its other lerp formula
    (end - (end - start) * (1 - weight)). That is outside the kernel's documented contract.
  * The sum of squares is formed here in fp64 and rounded once; torch and the kernel sum in fp32 in
    their own orders. The three agree whenever the sum is exact in fp32 in any order (entries +-2^k
    over a small range of k: pow4_gradient below); otherwise the norm may differ in the last place
    and a test has to search the neighbouring coefficients.
  * torch computes the coefficient as reciprocal(norm + 1e-6) * max_norm, and clip_grad_norm_ takes
    the norm of the per-tensor norms. Both equal the formulas above when max_norm is a power of two
    (1.0 is the project's only value, 0.5 the tests' other one) and every tensor's own sum of
    squares is a power of four (pow4_gradient), which is how the host test draws its gradients.
"""
import math

import numpy as np

f32 = np.float32


def fma32(a, b, c):
    """Correctly rounded fp32 a * b + c of fp32 arrays (Python 3.10 has no math.fma).
    The fp64 product of two fp32 numbers is exact (48 significant bits). TwoSum gives the fp64 sum s
    and its exact residual e (s + e = a * b + c). Rounding s straight to fp32 could round twice, so s
    is first moved to the neighbouring fp64 with an odd last bit whenever e != 0 (round to odd): an
    apparent fp32 tie in s is then broken by the residual's sign, and the final rounding to fp32 is
    the single rounding of the exact value."""
    a, b, c = (np.asarray(x, dtype=f32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (np.atleast_1d(s).view(np.int64) & 1) == 0
    fix = even.reshape(np.shape(s)) & (e != 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def adam_scalars(t, lr, beta1=0.9, beta2=0.999):
    """(nss, bc2s) of step t (the count after the increment): formed in double, rounded to fp32
    once each. lr may be an array (per-element learning rates) -> nss of the same shape."""
    t = float(t)
    bc1 = 1.0 - math.pow(beta1, t)
    bc2 = 1.0 - math.pow(beta2, t)
    nss = (-(np.asarray(lr, dtype=np.float64) / bc1)).astype(f32)
    return nss, f32(math.sqrt(bc2))


def grad_norm(g):
    """fp32 sqrt of the sum of squares (the sum in fp64, rounded to fp32 once: see the module
    docstring)."""
    g = np.asarray(g, dtype=f32).astype(np.float64)
    return np.sqrt(f32(np.sum(g * g)))


def clip_coef(norm, max_norm=1.0):
    return min(f32(max_norm) / (f32(norm) + f32(1e-6)), f32(1.0))


def clip_adam_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, coef=None, nss=None,
                   bc2s=None, fused_v=True, sqrt=np.sqrt):
    """One step on flat fp32 arrays -> (clipped g, m, v, p, coef). t is the step count after the
    increment; lr a scalar or a per-element array. coef / nss / bc2s override the model's own values
    (a test that searches the device's last-place choices passes them). fused_v=False computes v
    unfused, v * b2 + (w2 * g) * g with every operation rounded: NOT torch's arithmetic, kept to show
    that the bitwise tests tell the two apart. sqrt: the fp32 square root of denom (numpy's is
    correctly rounded, as the kernel's sqrtf; torch's CPU sqrt is not: the host test)."""
    p, g, m, v = (np.asarray(x, dtype=f32) for x in (p, g, m, v))
    if coef is None:
        coef = clip_coef(grad_norm(g), max_norm)
    coef = f32(coef)
    nss0, bc2s0 = adam_scalars(t, lr, beta1, beta2)
    nss = nss0 if nss is None else np.asarray(nss, dtype=f32)
    bc2s = bc2s0 if bc2s is None else f32(bc2s)
    w1, b2, w2, epsf = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps)
    g = g * coef
    m = fma32(w1, g - m, m)
    if fused_v:
        v = fma32(w2 * g, g, v * b2)
    else:
        v = v * b2 + (w2 * g) * g
    denom = sqrt(v) / bc2s + epsf
    p = p + (nss * m) / denom
    return g, m, v, p, coef


def pow4_gradient(rng, n, log4_sumsq):
    """n fp32 entries, each 0 or +-2^k, whose squares sum to 4^log4_sumsq exactly, in any order and
    in fp32: start from the single term 4^J and split random terms into four of the next lower power
    (at most 11 levels deep, so every partial sum is a multiple of the smallest term below 2^24 of
    it). The number of non-zero entries is 1 mod 3; the one or two entries left over are zeros."""
    nz = n - (n - 1) % 3
    depth = [0]
    open_ = [0]  # indices that may still split
    pick = iter(rng.random((nz - 1) // 3))
    while len(depth) < nz:
        if not open_:
            raise ValueError("pow4_gradient: n too large for 11 levels")
        i = int(next(pick) * len(open_))
        open_[i], open_[-1] = open_[-1], open_[i]
        j = open_.pop()
        d = depth[j] + 1
        depth[j] = d
        first = len(depth)
        depth.extend([d, d, d])
        if d < 11:
            open_.extend([j, first, first + 1, first + 2])
    k = np.full(n, np.nan)
    k[:nz] = log4_sumsq - np.asarray(depth, dtype=np.float64)
    mag = np.where(np.isnan(k), 0.0, np.exp2(np.nan_to_num(k)))
    out = (mag * rng.choice([-1.0, 1.0], size=n)).astype(f32)
    return out[rng.permutation(n)]
