#!/usr/bin/env python3
"""Pricing of the rollout with the critic off the step chain, one process, one GPU, HIP events around
single launches, the two variants alternating launch by launch on twin envs (same seeds):

  rollout  uavhip_rollout_steps, T steps of E x N x M (actor + critic in every step): us per step
  actor    uavhip_rollout_actor_steps, the same steps with the actor alone: us per step
  value    uavhip_value_steps over the T + 1 recorded windows (bootstrap included): us per step (/ T)
  bootstrap  uavhip_policy_value_rows, the launch the value pass makes unnecessary: us per launch

and the agreement of the two variants after every launch: trajectory and env state bitwise, values
as the largest absolute difference. Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "target-allocation-ppo-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from uavhip import TransformerActorCritic, VecUAVEnv
    from uavhip.policy import rowproj_buffer
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    net = TransformerActorCritic().to(dev)
    net.packed_weights()
    E, N, M, T = a.envs, a.uavs, a.targets, a.steps

    class Side:
        def __init__(self):
            self.env = VecUAVEnv(E, N, M, seed=1)
            self.env.istate[:, 4] = 1
            self.env.generate_scenes()
            self.obs = torch.zeros(T + 1, E, 5, 14, device=dev)
            self.env.reset(episode=1, obs_out=self.obs[0])
            self.rp = rowproj_buffer(E, dev)
            self.act = torch.zeros(T, E, dtype=torch.int8, device=dev)
            self.lp, self.val = torch.zeros(T, E, device=dev), torch.zeros(T, E, device=dev)
            self.last = torch.zeros(E, device=dev)
            self.rew = torch.zeros(T, E, dtype=torch.float64, device=dev)
            self.dn = torch.zeros(T, E, dtype=torch.uint8, device=dev)

    A, B = Side(), Side()
    names = ("rollout", "bootstrap", "actor", "value")
    ev = {k: [] for k in names}

    def timed(k, on, fn):
        if not on:
            return fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        ev[k].append((s, e))

    same, vdiff = True, 0.0
    for i in range(a.warmup + a.launches):
        on = i >= a.warmup
        kw = dict(seed=7, offset=i * (T + 1) * E, offset_stride=E)
        for s in (A, B):
            if i:
                s.obs[0].copy_(s.obs[T])
        timed("rollout", on, lambda: net.rollout_steps(A.env, A.obs, A.rp, 0, True, A.act, A.lp, A.val, A.rew, A.dn,
                                                       None, **kw))
        timed("bootstrap", on, lambda: net.value_rows(A.obs[T], A.rp, T, A.last))
        timed("actor", on, lambda: net.rollout_actor_steps(B.env, B.obs, B.rp, 0, True, B.act, B.lp, B.rew, B.dn,
                                                           None, **kw))
        timed("value", on, lambda: net.value_steps(B.obs, B.rp, 0, B.val, B.last))
        for s in (A, B):
            s.env.refresh_scenes()
        same = same and all(torch.equal(getattr(A, n), getattr(B, n)) for n in ("obs", "act", "lp", "rew", "dn")) and \
            torch.equal(A.env.dstate, B.env.dstate) and torch.equal(A.env.istate, B.env.istate)
        vdiff = max(vdiff, float((A.val - B.val).abs().max()), float((A.last - B.last).abs().max()))
    torch.cuda.synchronize()
    assert int(A.env.errors().max()) == 0 and int(B.env.errors().max()) == 0

    def stats(k, div):
        us = sorted(1e3 * s.elapsed_time(e) / div for s, e in ev[k])
        return {"median": us[len(us) // 2], "min": us[0], "max": us[-1]}

    out = {"workload": f"{E} x {N} x {M}", "steps_per_launch": T, "launches": a.launches,
           "device": torch.cuda.get_device_name(0),
           "rollout_us_per_step": stats("rollout", T), "bootstrap_us_per_launch": stats("bootstrap", 1),
           "actor_us_per_step": stats("actor", T), "value_us_per_step": stats("value", T),
           "trajectory_and_env_state_bitwise_equal": bool(same), "values_max_abs_diff": vdiff,
           "dones_per_launch": float(A.dn.sum())}
    out["deferred_minus_fused_us_per_iteration"] = T * (out["actor_us_per_step"]["median"] +
                                                        out["value_us_per_step"]["median"] -
                                                        out["rollout_us_per_step"]["median"]) - \
        out["bootstrap_us_per_launch"]["median"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
