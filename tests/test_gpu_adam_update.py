"""GPU: the UPDATE phase alone (k_grad_norm + k_adam, csrc/train.hip) against tests/adam_model.py, the
numpy restatement of clip_grad_norm_ + torch's single-tensor Adam that tests/test_adam_model_host.py
pins to torch on the CPU. Marked gpu.

Every case writes chosen parameters, gradients, moments and step count into a FusedPPOTrainer's flat
buffers (real elements only: the padding between tensors stays zero, k_grad_norm sums all n_floats),
calls step(PPO_UPDATE) and requires, bit for bit over every element:
  * grads = fl(g * c) for ONE fp32 coefficient c: the model's own when the norm is order-independent
    (gradients +-2^k, adam_model.pow4_gradient), else one of the fp32 values within 4 ulp of the
    coefficient from the fp64 norm (the kernel sums g^2 in fp32 over 256 blocks);
  * adam_m and adam_v are the model's given c;
  * params is the model's for one choice of (nss_actor, nss_critic, bc2s) among the host's values
    and their +-1 ulp fp32 neighbours (the device's double pow is not guaranteed correctly rounded),
    the same choice for every element of a group; at t = 1 with the default hyper-parameters the choice
    must be the host's own;
  * adam_step advanced by exactly 1, the padding is still zero, nothing is non-finite.
The per-element learning rate comes from the state-dict key names (actor* / critic*), not from the
kernel's tables. Each case prints its mismatch counts and choices before it asserts.

Measured on the MI355X: the build before this file computed v unfused and took the
root with __fsqrt_rn, which is the native 1-ulp v_sqrt_f32 in this toolchain; of 419 267 elements
per step adam_v was off in 1 770 to 7 780 (clip active, non-zero v) and params in 428 to 3 783. With v
as one fma and sqrtf every count is 0, the coefficient is the fp64 norm's own (0 ulp) also for random
gradients, and the three scalars are the host's own in every case.

Subnormals are avoided on purpose (the tiny-gradient case uses magnitudes whose squares are either
normal or underflow to zero outright): the denormal mode of a kernel is a build setting, not part of
the update's contract.
"""
import numpy as np
import pytest
import torch

import adam_model as am
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEFAULT = dict(lr_actor=2e-4, lr_critic=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _ulps(x, k):
    """fp32 x moved k places (x finite, non-zero)."""
    return (np.asarray(x, dtype=np.float32).view(np.int32) + np.int32(k)).view(np.float32)


class Update:
    """A trainer whose UPDATE phase runs alone, with the host-side picture of its flat layout."""

    def __init__(self, **hyper):
        from uavhip.policy import TransformerActorCritic, layout
        from uavhip.train import FusedPPOTrainer
        self.h = dict(DEFAULT, **hyper)
        torch.manual_seed(0)
        policy = TransformerActorCritic().cuda()
        h = self.h
        self.tr = FusedPPOTrainer(policy, 64, lr_actor=h["lr_actor"], lr_critic=h["lr_critic"],
                                  betas=(h["beta1"], h["beta2"]), adam_eps=h["eps"], max_grad_norm=h["max_norm"])
        z = torch.zeros
        self.tr.set_buffers(z(64, 5, 14), z(64, dtype=torch.int8), z(64), z(64), z(64), z(64))  # never read by UPDATE
        offs, self.n = layout()
        sd = policy.state_dict()
        assert len(sd) == len(offs)
        self.real = np.zeros(self.n, bool)
        self.lr = np.full(self.n, h["lr_actor"])  # padding: zeros in every buffer, any rate does
        self.first_critic = None
        for (k, p), o in zip(sd.items(), offs):
            self.real[o:o + p.numel()] = True
            if k.startswith("critic"):
                self.lr[o:o + p.numel()] = h["lr_critic"]
                if self.first_critic is None:
                    self.first_critic = o
            else:
                assert k.startswith("actor"), k
        assert self.lr[self.first_critic] == h["lr_critic"] and self.lr[self.first_critic - 1] == h["lr_actor"]
        self.idx = np.nonzero(self.real)[0]
        self.actor = self.lr == h["lr_actor"]

    def full(self, values):
        """Real-element values -> a flat [n_floats] fp32 array with zero padding."""
        out = np.zeros(self.n, np.float32)
        out[self.idx] = values
        return out

    def state(self):
        tr = self.tr
        torch.cuda.synchronize()
        return tuple(x.cpu().numpy().copy() for x in (tr.params, tr.grads, tr.adam_m, tr.adam_v)) + \
            (float(tr.adam_step.item()),)

    def run(self, label, g, p=None, m=None, v=None, t0=None, exact_norm=True):
        """Write the given buffers (None: keep the device's), run UPDATE, compare with the model.
        -> dict of mismatch counts and choices (printed first, asserted after)."""
        from uavhip import _lib
        tr = self.tr
        for buf, x in ((tr.params, p), (tr.grads, g), (tr.adam_m, m), (tr.adam_v, v)):
            if x is not None:
                buf.copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
        if t0 is not None:
            tr.adam_step.fill_(float(t0))
        p0, g0, m0, v0, t0 = self.state()
        tr.step(_lib.PPO_UPDATE)
        p1, g1, m1, v1, t1 = self.state()
        h, t = self.h, t0 + 1.0
        kw = dict(beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], max_norm=h["max_norm"])
        # --- the coefficient
        c0 = am.clip_coef(am.grad_norm(g0), h["max_norm"])
        cands = [0] if exact_norm else [0, -1, 1, -2, 2, -3, 3, -4, 4]
        c_off, g_bad = None, None
        for k in cands:
            c = np.float32(min(_ulps(c0, k), np.float32(1.0)))
            bad = int(np.count_nonzero(_bits(g0 * c) != _bits(g1)))
            if g_bad is None or bad < g_bad:
                c_off, g_bad, coef = k, bad, c
            if bad == 0:
                break
        # --- moments given the coefficient; parameters for the host's scalars, else their neighbours
        nss0, bc2s0 = am.adam_scalars(t, self.lr, h["beta1"], h["beta2"])
        nss_a, nss_c = nss0[self.actor][0], nss0[~self.actor][0]

        def model(da, dc, db):
            nss = np.where(self.actor, _ulps(nss_a, da), _ulps(nss_c, dc))
            return am.clip_adam_step(p0, g0, m0, v0, t, self.lr, coef=coef, nss=nss, bc2s=_ulps(bc2s0, db), **kw)
        _, m_m, v_m, p_m, _ = model(0, 0, 0)
        m_bad = int(np.count_nonzero(_bits(m_m) != _bits(m1)))
        v_bad = int(np.count_nonzero(_bits(v_m) != _bits(v1)))
        p_off = _bits(p_m) != _bits(p1)
        choice = (0, 0, 0)
        if p_off.any():  # the same bc2s for both groups, one nss per group
            best = (int(p_off.sum()), choice)
            for db in (0, -1, 1):
                pa = {da: _bits(model(da, 0, db)[3]) != _bits(p1) for da in (0, -1, 1)}
                pc = {dc: _bits(model(0, dc, db)[3]) != _bits(p1) for dc in (0, -1, 1)}
                for da in (0, -1, 1):
                    for dc in (0, -1, 1):
                        bad = int((pa[da] & self.actor).sum() + (pc[dc] & ~self.actor).sum())
                        if bad < best[0]:
                            best = (bad, (da, dc, db))
            p_bad, choice = best
        else:
            p_bad = 0
        pad_bad = int(sum(np.count_nonzero(x[~self.real]) for x in (p1, g1, m1, v1)))
        finite = all(np.isfinite(x).all() for x in (p1, g1, m1, v1))
        res = dict(t=t, coef=float(coef), coef_ulps_from_fp64_norm=c_off, g_bad=g_bad, m_bad=m_bad, v_bad=v_bad,
                   p_bad=p_bad, scalar_choice_ulps=choice, pad_bad=pad_bad, finite=finite, t1=t1)
        print(f"{label}: {res}")
        assert t1 == t
        assert finite
        assert pad_bad == 0
        assert g_bad == 0, "grads is not fl(g * c) for one coefficient"
        assert m_bad == 0, "adam_m"
        assert v_bad == 0, "adam_v"
        assert p_bad == 0, "params"
        if t == 1.0 and h == DEFAULT:
            assert choice == (0, 0, 0)
        self.out = (p0, g0, m0, v0, p1, g1, m1, v1)
        return res


@pytest.fixture(scope="module")
def up():
    return Update()


@pytest.fixture(scope="module")
def base(up):
    """One +-2^k pattern over the real elements with sum of squares exactly 1; the cases permute it,
    flip signs and scale it by powers of two (all exact)."""
    return am.pow4_gradient(np.random.default_rng(7), len(up.idx), 0)


def _grad(up, base, rng, log2_norm):
    g = base[rng.permutation(len(base))] * rng.choice([-1.0, 1.0], size=len(base)).astype(np.float32)
    return up.full(g * np.float32(2.0 ** log2_norm))


def _moments(up, rng, m_scale=1e-3):
    m = up.full(rng.normal(size=len(up.idx)) * m_scale)
    v = up.full((rng.normal(size=len(up.idx)) * m_scale) ** 2)
    return m, v


def test_fresh_state_clip_inactive(up, base):
    """t = 1 from zero moments, norm 0.5: the coefficient is exactly 1, the gradients come back
    unchanged, and the step is the closed form -lr g / (|g| + eps) (m / (1 - b1) = g,
    sqrt(v / (1 - b2)) = |g| up to a few roundings): an independent check on the model."""
    rng = np.random.default_rng(1)
    g = _grad(up, base, rng, -1)
    p = up.full(rng.normal(size=len(up.idx)) * 0.1)
    res = up.run("fresh", g, p=p, m=np.zeros_like(g), v=np.zeros_like(g), t0=0)
    p0, g0, _, _, p1, g1, _, _ = up.out
    assert res["coef"] == 1.0
    assert np.array_equal(_bits(g1), _bits(g0))
    want = -up.lr * g0.astype(np.float64) / (np.abs(g0.astype(np.float64)) + 1e-8)
    got = p1.astype(np.float64) - p0.astype(np.float64)
    # the step itself to 1e-4 relative (fp32 roundings of a few operations), plus p's own rounding
    tol = 1e-4 * up.lr + 2.0 ** -23 * np.abs(p0)
    err = np.abs(got - want)
    print(f"closed form: max |dp - want| / lr = {(err / up.lr).max():.3e}")
    assert (err <= tol).all()


def test_clip_active(up, base):
    rng = np.random.default_rng(2)
    m, v = _moments(up, rng)
    res = up.run("clip active (norm 8)", _grad(up, base, rng, 3), p=up.full(rng.normal(size=len(up.idx)) * 0.1),
                 m=m, v=v, t0=4)
    assert res["coef"] == float(np.float32(1.0) / (np.float32(8.0) + np.float32(1e-6)))


def test_norm_at_max_norm(up, base):
    """norm = max_norm exactly: the 1e-6 term alone makes the coefficient 1 / (1 + 8 ulp) < 1."""
    rng = np.random.default_rng(3)
    m, v = _moments(up, rng)
    res = up.run("norm = max_norm", _grad(up, base, rng, 0), p=up.full(rng.normal(size=len(up.idx)) * 0.1),
                 m=m, v=v, t0=4)
    assert res["coef"] < 1.0 and res["coef"] == float(np.float32(1.0) / (np.float32(1.0) + np.float32(1e-6)))


def test_zero_gradient_zero_moments(up):
    """0 / eps, not NaN: nothing moves."""
    rng = np.random.default_rng(4)
    z = np.zeros(up.n, np.float32)
    p = up.full(rng.normal(size=len(up.idx)) * 0.1)
    up.run("zero gradient, zero moments", z, p=p, m=z, v=z, t0=0)
    p0, _, _, _, p1, g1, m1, v1 = up.out
    assert np.array_equal(_bits(p1), _bits(p0))
    assert not g1.any() and not m1.any() and not v1.any()


def test_zero_gradient_decays_moments(up):
    """The moments decay (m by 1 - w1, v by b2) and the parameters move on m alone."""
    rng = np.random.default_rng(5)
    m, v = _moments(up, rng)
    up.run("zero gradient, moments", np.zeros(up.n, np.float32), p=up.full(rng.normal(size=len(up.idx)) * 0.1),
           m=m, v=v, t0=7)
    p0, _, m0, v0, p1, _, m1, v1 = up.out
    r = up.real & (m0 != 0) & (v0 > 0)
    assert (np.abs(m1[r]) < np.abs(m0[r])).all() and (v1[r] < v0[r]).all()
    moved = np.sign(p1[r].astype(np.float64) - p0[r])  # 0 where the step is below half an ulp of p
    assert ((moved == -np.sign(m0[r])) | (moved == 0)).all() and (moved != 0).mean() > 0.9


def test_six_steps_alternating_clip(up, base):
    """Six launches, clip active and inactive in turn, each from the kernel's own previous outputs;
    the model restarts from the same inputs every step, so one mismatch would not cascade."""
    rng = np.random.default_rng(6)
    z = np.zeros(up.n, np.float32)
    for s in range(6):
        g = _grad(up, base, rng, 3 if s % 2 == 0 else -1)
        first = s == 0
        res = up.run(f"sequence step {s + 1}", g, p=up.full(rng.normal(size=len(up.idx)) * 0.1) if first else None,
                     m=z if first else None, v=z if first else None, t0=0 if first else None)
        assert res["t"] == s + 1 and (res["coef"] < 0.2) == (s % 2 == 0)


@pytest.mark.parametrize("t0", [1e4, 1e6])
def test_large_step_counts(up, base, t0):
    """b1^t underflows (bias correction 1 exactly 1); b2^t is 4.5e-5 at 1e4 and underflows at 1e6."""
    rng = np.random.default_rng(8)
    m, v = _moments(up, rng)
    res = up.run(f"adam_step {t0:g}", _grad(up, base, rng, 2), p=up.full(rng.normal(size=len(up.idx)) * 0.1),
                 m=m, v=v, t0=t0)
    assert res["t"] == t0 + 1


def test_tiny_gradients_beside_ordinary_moments(up):
    """|g| = 2^-40 (squares normal, also after w2) and 2^-83 (about 1e-25: w2 g is normal, its product
    with g underflows to zero outright), a third of the elements with zero moments, the rest O(1)."""
    rng = np.random.default_rng(9)
    n = len(up.idx)
    g = np.where(rng.random(n) < 0.5, 2.0 ** -40, 2.0 ** -83) * rng.choice([-1.0, 1.0], size=n)
    m = rng.normal(size=n)
    v = rng.normal(size=n) ** 2 + 0.01
    cold = rng.random(n) < 1 / 3
    m[cold] = 0.0
    v[cold] = 0.0
    res = up.run("tiny gradients", up.full(g), p=up.full(rng.normal(size=n) * 0.1), m=up.full(m), v=up.full(v), t0=5,
                 exact_norm=False)
    assert res["coef"] == 1.0


def test_random_normal_gradients(up):
    """Ordinary gradients (norm about 6.5: clip active): the kernel's fp32 norm may differ from the
    fp64 one in the last place, so the coefficient is searched among the neighbours and printed."""
    rng = np.random.default_rng(10)
    n = len(up.idx)
    m, v = _moments(up, rng)
    res = up.run("random normal gradients", up.full(rng.normal(size=n) * 0.01), p=up.full(rng.normal(size=n) * 0.1),
                 m=m, v=v, t0=10, exact_norm=False)
    assert 0.1 < res["coef"] < 0.2


def test_non_default_hyper_parameters(base):
    """beta1 0.8, adam_eps 1e-5, max_grad_norm 0.5: the descriptor carries all three."""
    u = Update(beta1=0.8, eps=1e-5, max_norm=0.5)
    rng = np.random.default_rng(11)
    m, v = _moments(u, rng)
    res = u.run("beta1 0.8, eps 1e-5, max_norm 0.5", _grad(u, base, rng, 1),
                p=u.full(rng.normal(size=len(u.idx)) * 0.1), m=m, v=v, t0=3)
    assert res["coef"] == float(np.float32(0.5) / (np.float32(2.0) + np.float32(1e-6)))
