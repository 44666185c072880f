#!/usr/bin/env python3
"""Inference timing: the actor-only decode kernel beside the training rollout kernel, and the
throughput of a full best-of-K solve. One process, one GPU, HIP events around single launches.

  rollout  uavhip_rollout_steps, T = 64 steps of 4096 x 16 x 32 (actor + critic, logp / value,
           trajectory stores, auto-reset): us per step
  decode   uavhip_decode_steps, n_max = 64 steps of the same envs, freshly reset before every launch:
           us per step, greedy (the initial policy skips at every step, so no env finishes and every
           workgroup runs all 64 steps) and with every env sampling (greedy_stride = 0: the envs end
           after ~2 N steps and the workgroups leave early; per step of the launch's longest env, the
           finished envs counted)
  ratio    decode / rollout per step: what is left of the step's serial chain without the critic
  solve    AllocationSolver.solve over 4096 on-device scenes at K = 1 (greedy) and K = 8 (replica 0
           greedy, 7 sampled), wall time around the call incl. scene generation, reset, decode to the
           episode ends and uavhip_select_best: scenes/s

The policy is the seeded initial policy (no trained checkpoint ships with the repository): greedy, it
skips at every step, so a K = 1 solve decodes the longest possible episode (N * M = 512 steps) --
the worst case for scenes/s. Prints one JSON line; --out also writes it to a file
(profiles/solve_bench.json is a recorded run).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "target-allocation-ppo-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64, help="steps per launch (T / n_max)")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--solves", type=int, default=3, help="timed solves per K")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from uavhip import AllocationSolver, TransformerActorCritic, VecUAVEnv
    from uavhip.policy import rowproj_buffer
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    net = TransformerActorCritic().to(dev)
    net.packed_weights()
    E, N, M, T = a.envs, a.uavs, a.targets, a.steps

    def events(n):
        return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]

    def per_step_us(ev):
        ms = sorted(s.elapsed_time(e) for s, e in ev)
        return {"median": 1e3 * ms[len(ms) // 2] / T, "min": 1e3 * ms[0] / T, "max": 1e3 * ms[-1] / T}

    # ---- the training rollout kernel
    env = VecUAVEnv(E, N, M, seed=1)
    env.istate[:, 4] = 1
    env.generate_scenes()
    obs = torch.zeros(T + 1, E, 5, 14, device=dev)
    env.reset(episode=1, obs_out=obs[0])
    rp = rowproj_buffer(E, dev)
    act = torch.zeros(T, E, dtype=torch.int8, device=dev)
    lp, val = torch.zeros(T, E, device=dev), torch.zeros(T, E, device=dev)
    rew = torch.zeros(T, E, dtype=torch.float64, device=dev)
    dn = torch.zeros(T, E, dtype=torch.uint8, device=dev)
    ev = events(a.launches)
    for i in range(a.warmup + a.launches):
        if i:
            obs[0].copy_(obs[T])  # the next iteration starts from the last windows
        j = i - a.warmup
        if j >= 0:
            ev[j][0].record()
        net.rollout_steps(env, obs, rp, 0, True, act, lp, val, rew, dn, None, seed=7, offset=i * T * E, offset_stride=E)
        if j >= 0:
            ev[j][1].record()
        env.refresh_scenes()
    torch.cuda.synchronize()
    rollout = per_step_us(ev)

    # ---- the decode kernel: the same shape, fresh episodes in every launch. Greedy, the initial policy
    # skips at every step: no env finishes inside T steps and every workgroup runs all T -- the
    # per-step figure the ratio uses. Sampling (greedy_stride = 0), an env ends after ~2 N steps and the
    # workgroups leave early: that launch is normalised by the steps of its longest env, and the
    # finished envs are counted.
    denv = VecUAVEnv(E, N, M, seed=1, full_reset_period=0)
    denv.generate_scenes()
    obs2 = torch.zeros(2, E, 5, 14, device=dev)
    steps = torch.zeros(E, dtype=torch.int32, device=dev)
    fin = torch.zeros(E, dtype=torch.uint8, device=dev)
    ret = torch.zeros(E, dtype=torch.float64, device=dev)

    def time_decode(greedy_stride):
        ev = events(a.launches)
        finished, longest = [], []
        for i in range(a.warmup + a.launches):
            denv.reset(episode=1, obs_out=obs2[0])
            steps.zero_()
            ret.zero_()
            j = i - a.warmup
            if j >= 0:
                ev[j][0].record()
            net.decode_steps(denv, obs2, rp, 0, True, steps, fin, ep_return=ret, n_max=T, greedy_stride=greedy_stride,
                             seed=7, offset=i * T * E, offset_stride=E)
            if j >= 0:
                ev[j][1].record()
                finished.append(fin.sum())
                longest.append(steps.max())
        torch.cuda.synchronize()
        ms = [s.elapsed_time(e) for s, e in ev]
        us = sorted(1e3 * m / int(n) for m, n in zip(ms, longest))  # per step of the launch's longest env
        return {"median": us[len(us) // 2], "min": us[0], "max": us[-1], "launch_ms_median": sorted(ms)[len(ms) // 2],
                "finished_envs_mean": float(torch.stack(finished).double().mean()),
                "longest_env_steps_mean": float(torch.stack(longest).double().mean())}

    decode = time_decode(1)
    decode_sampling = time_decode(0)
    assert int(denv.errors().max()) == 0

    # ---- full solves
    solve = {}
    for K in (1, 8):
        solver = AllocationSolver(net, N, M, samples=K)
        solver.solve(num_scenes=E, seed=0)
        torch.cuda.synchronize()
        best = None
        for i in range(a.solves):
            t0 = time.perf_counter()
            r = solver.solve(num_scenes=E, seed=i)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        solve[f"K{K}"] = {"scenes_per_s": E / best, "ms": 1e3 * best, "mean_steps": float(r.steps.double().mean()),
                          "max_replica_steps": int(solver.steps.max()), "mean_J": float(r.J.mean()),
                          "unfinished": int((r.best_replica < 0).sum())}
        del solver
    out = {"workload": f"{E} x {N} x {M}", "steps_per_launch": T, "launches": a.launches,
           "device": torch.cuda.get_device_name(0), "policy": "seeded initial policy (torch.manual_seed(0))",
           "rollout_us_per_step": rollout, "decode_us_per_step": decode,
           "decode_sampling_us_per_step": decode_sampling,
           "decode_over_rollout": decode["median"] / rollout["median"], "solve": solve}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
