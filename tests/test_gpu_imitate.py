"""uavhip.imitate on the GPU: teacher_batch's returns against the numpy fp32 recursion, the update's
gradient against fp64 autograd of the likelihood loss it stands for, an update that lowers the
negative log-likelihood, ImitationRun's seeding contract and files, and uavhip.fit --init.
64 envs x 4 x 4, minibatch 64."""
import json

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

E, N, M, MB = 64, 4, 4, 64


def scene_env(seed):
    from uavhip.vec_env import VecUAVEnv
    env = VecUAVEnv(E, N, M, seed=seed, full_reset_period=0, scene_buffers=1)
    env.generate_scenes()
    return env


@pytest.fixture(scope="module")
def batch():
    from uavhip.imitate import teacher_batch
    b = teacher_batch(scene_env(5))
    torch.cuda.synchronize()
    return b


def test_batch_shapes_and_returns_vs_recursion(batch):
    """returns = r_t + gamma (1 - done_t) ret_{t+1} in fp32, 0 in held rows: bit for bit oracle/gae.py
    with lambda = 1 and zero values (as test_gae_vs_reference holds GAE's returns)."""
    from oracle import gae as ogae
    from uavhip.config import cfg
    from uavhip.imitate import teacher_batch
    T = N * M
    assert batch.obs.shape == (T, E, 5, 14) and batch.actions.shape == (T, E) and batch.returns.shape == (T, E)
    assert batch.returns.dtype == torch.float32 and batch.rows.dtype == torch.int32
    valid = batch.actions.reshape(-1) >= 0
    assert torch.equal(batch.rows.long(), torch.nonzero(valid).reshape(-1))
    assert int(batch.rows.numel()) == int(batch.steps.sum()) and bool((batch.steps >= N).all())
    assert not bool(batch.returns.reshape(-1)[~valid].any())
    # the baseline teacher is walked as it is unless the env rejects an assign
    same = batch.rejected == 0
    assert bool(same.any())
    gap = ((batch.J - batch.teacher_J).abs() / batch.teacher_J.abs().clamp(min=1.0))[same].max().item()
    print(f"{int(batch.rows.numel())} rows, mean teacher J {batch.teacher_J.mean().item():.4f}, walked "
          f"{batch.J.mean().item():.4f}, {int(batch.rejected.sum())} rejected, max J gap where none {gap:.2e}")
    assert gap <= 1e-12
    # the recursion, on the kernel's own rewards
    env = scene_env(5)
    again = teacher_batch(env)
    env.reset()
    out = env.teacher_steps(env.refine_assignments(None)[0])
    torch.cuda.synchronize()
    assert torch.equal(again.returns, batch.returns) and torch.equal(again.actions, batch.actions)
    assert torch.equal(out["actions"], batch.actions)
    rew, done = out["reward"].cpu().numpy(), out["done"].cpu().numpy()
    want, _ = ogae.gae_2d(rew, done, np.zeros((T, E), np.float32), gamma=cfg.GAMMA, lam=1.0)
    assert np.array_equal(batch.returns.cpu().numpy(), want)
    assert float(np.abs(want).max()) > 0


def _likelihood_loss(policy, states, acts, ret, value_coef=0.5, entropy_coef=0.01):
    lp, v, ent = policy.evaluate(states, acts)
    v = torch.squeeze(v)
    return -lp.mean() + value_coef * ((v - ret) ** 2).mean() - entropy_coef * ent.mean()


def test_update_gradient_is_the_likelihood_gradient(batch):
    """One FORWARD | BACKWARD step on imitation_update's own buffers against fp64 autograd of
    -mean log pi(a*) + value_coef mean (v - R)^2 - entropy_coef mean H. The bar is
    test_gradients_per_element_vs_fp64's (tests/test_gpu_train.py), restated: per element with
    |ref| >= 1e-3 of its tensor's max, |hip - ref64| <= 2e-4 |ref64| + 1e-7 max|ref| or no more than
    twice torch fp32's error there + 2e-6 |ref64|; and p99 of the relative error <= 2 x torch fp32's
    + 1e-6."""
    from uavhip.imitate import build_batch
    from uavhip.policy import TransformerActorCritic, layout
    from uavhip.train import FusedPPOTrainer
    torch.manual_seed(31)
    net = TransformerActorCritic().cuda()
    tr = FusedPPOTrainer(net, MB)
    bufs, k, _ = build_batch(net, batch, pad_to=MB)
    assert k == int(batch.rows.numel()) and bufs[0].shape[0] % MB == 0 and bufs[0].shape[0] - k < MB
    states, acts, old_logp, old_values, ret, adv = bufs
    assert bool((adv[:k] == 1.0).all()) and acts.dtype == torch.int8
    idx = torch.randperm(k, generator=torch.Generator().manual_seed(33))[:MB]
    assert 0 < int(acts[idx.cuda()].sum()) < MB  # both actions in the minibatch
    tr.set_buffers(*bufs)
    grads = tr.gradients(idx.cuda()).double().cpu()
    sd = {n_: v.detach().cpu().clone() for n_, v in net.state_dict().items()}
    s, a, r = states[idx.cuda()].cpu(), acts[idx.cuda()].long().cpu(), ret[idx.cuda()].cpu()
    ref64, ref32 = TransformerActorCritic().double(), TransformerActorCritic()
    ref64.load_state_dict({n_: v.double() for n_, v in sd.items()})
    ref32.load_state_dict(sd)
    _likelihood_loss(ref64, s.double(), a, r.double()).backward()
    _likelihood_loss(ref32, s, a, r).backward()
    offs, _ = layout()
    bad, rels_h, rels_t, n_second = [], [], [], 0
    for (name, p32), p64, o in zip(ref32.named_parameters(), ref64.parameters(), offs):
        ref = p64.grad.reshape(-1)
        got = grads[o:o + p32.numel()]
        t32 = p32.grad.reshape(-1).double()
        scale = float(ref.abs().max())
        sel = ref.abs() >= 1e-3 * scale
        if not bool(sel.any()):
            continue
        tol = 2e-4 * ref.abs() + 1e-7 * scale
        eh, et = (got - ref).abs(), (t32 - ref).abs()
        first = eh <= tol
        second = eh <= 2 * et + 2e-6 * ref.abs()
        rels_h.append((eh / ref.abs())[sel])
        rels_t.append((et / ref.abs())[sel])
        n2 = int((sel & ~first & second).sum())
        n_second += n2
        print(f"{name}: {int(sel.sum())}/{ref.numel()} elements, max rel {float(rels_h[-1].max()):.2e} (torch fp32 "
              f"{float(rels_t[-1].max()):.2e}), bar use {float((eh / tol)[sel].max()):.3f}, {n2} by the fp32 clause")
        if bool((sel & ~first & ~second).any()):
            bad.append((name, int((sel & ~first & ~second).sum())))
    ph, pt = float(torch.cat(rels_h).quantile(0.99)), float(torch.cat(rels_t).quantile(0.99))
    print(f"p99 rel HIP {ph:.2e}, torch fp32 {pt:.2e}; {n_second} element(s) passed by the fp32-reference clause")
    assert bool(torch.isfinite(grads).all()), "non-finite gradient"
    assert not bad, f"elements outside both per-element bars: {bad}"
    assert ph <= 2 * pt + 1e-6, (ph, pt)


def test_update_lowers_the_nll_and_weights_assigns(batch):
    from uavhip.imitate import build_batch, imitation_update
    from uavhip.policy import TransformerActorCritic
    from uavhip.train import FusedPPOTrainer
    torch.manual_seed(7)
    net = TransformerActorCritic().cuda()
    tr = FusedPPOTrainer(net, MB)
    bufs, k, _ = build_batch(net, batch, assign_weight=3.0)
    assert bufs[0].shape[0] == k
    assert torch.equal(bufs[5], torch.where(bufs[1] == 1, 3.0, 1.0).float())
    off = net._sample_offset
    q = imitation_update(tr, net, batch, 5, torch.Generator().manual_seed(1))
    print(q)
    assert net._sample_offset == off  # the forwards ran counter-neutral
    assert q["rows"] == k and q["optimizer_steps"] == 5 * -(-k // MB)
    assert q["nll_after"] < q["nll_before"]
    assert 0.0 <= q["agreement_before"] <= 1.0 and 0.0 <= q["agreement"] <= 1.0


def test_runs_are_reproducible_and_feed_solve_and_fit(tmp_path, capsys):
    from uavhip import solve
    from uavhip.checkpoint import read_checkpoint
    from uavhip.fit import TrainingRun
    from uavhip.imitate import ImitationRun
    from uavhip.policy import layout
    a = ImitationRun(E, N, M, MB, str(tmp_path / "a"), seed=3, epochs=2, eval_every=2, eval_scenes=16)
    sa = a.fit(2)
    b = ImitationRun(E, N, M, MB, str(tmp_path / "b"), seed=3, epochs=2)
    b.fit(2)
    c = ImitationRun(E, N, M, MB, str(tmp_path / "c"), seed=4, epochs=2)
    c.fit(2)
    assert torch.equal(a.trainer.params, b.trainer.params)
    assert not torch.equal(a.trainer.params, c.trainer.params)
    lines = [json.loads(x) for x in open(tmp_path / "a" / "progress.jsonl")]
    assert [x["iteration"] for x in lines] == [1, 2]
    for x in lines:
        assert list(x)[:7] == ["iteration", "rows", "nll_before", "nll_after", "agreement", "teacher_mean_J", "rejected"]
    assert "eval_mean_J" not in lines[0] and {"eval_mean_J", "eval_mean_J_baseline", "eval_beats_baseline"} <= set(lines[1])
    assert lines[0]["rows"] != lines[1]["rows"] or lines[0]["teacher_mean_J"] != lines[1]["teacher_mean_J"]  # fresh scenes
    ck = sa["final_model"]
    sd = read_checkpoint(ck)
    assert len(sd) == 50
    for k, v in a.policy.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    capsys.readouterr()
    solve.main(["--checkpoint", ck, "--scenes", "8", "--samples", "2", "--uavs", str(N), "--targets", str(M)])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["scenes"] == 8 and out["unfinished"] == 0
    run = TrainingRun(E, N, M, 8, MB, str(tmp_path / "fit"), seed=0, init=ck)
    for k, v in run.policy.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    off, _ = layout()
    assert torch.equal(run.trainer.params[off[0]:off[0] + 8].cpu(), list(sd.values())[0].reshape(-1)[:8])
    f = run.step()
    assert f["iteration"] == 1 and f["optimizer_steps"] > 0
    assert not torch.equal(list(run.policy.state_dict().values())[0].cpu(), list(sd.values())[0])
    with pytest.raises(ValueError, match="init and resume"):
        TrainingRun(E, N, M, 8, MB, str(tmp_path / "fit"), seed=0, init=ck, resume=str(tmp_path / "fit"))
