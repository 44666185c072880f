#!/usr/bin/env python3
"""What the best-response local search (uavhip_refine_assignments) costs and buys, in
one process on one GPU at 4096 scenes x 16 x 32 with K = 8 replicas:

  solve0 / solve32 / baseline   wall time (host clock around the call, ending in a device synchronise)
           of AllocationSolver.solve(refine=0), solve(refine=32) and baseline() on the same on-device
           scenes, the three alternating, median and best of --solves rounds
  refine_launch / baseline_launch   the k_refine launch alone by HIP events: from the best-of-K
           assignment of a solve at env_stride = K, and from the empty assignment
  refine_over_solve0   the refine launch's median over solve0's median wall time
  J        mean J of the decoded, refined and baseline allocations, mean sweeps and moves, and the
           share of scenes where the policy beats the baseline

The policy is --checkpoint, or else the seeded initial policy (torch.manual_seed(0)): UNTRAINED, so
its J figures say nothing about a trained policy -- they only show the search at work. Prints one
JSON line; --out also writes it (profiles/refine_bench.json is a recorded run).
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
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=32)
    ap.add_argument("--solves", type=int, default=5, help="timed rounds of solve0 / solve32 / baseline")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from uavhip import AllocationSolver, TransformerActorCritic
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    net = TransformerActorCritic().to(dev)
    policy = "seeded initial policy (torch.manual_seed(0)), UNTRAINED"
    if a.checkpoint:
        from uavhip.checkpoint import load_checkpoint
        load_checkpoint(net, a.checkpoint)
        policy = os.path.basename(a.checkpoint)
    S, N, M, K = a.scenes, a.uavs, a.targets, a.samples
    solver = AllocationSolver(net, N, M, samples=K)
    calls = {"solve0": lambda: solver.solve(num_scenes=S, seed=0),
             "solve32": lambda: solver.solve(num_scenes=S, seed=0, refine=a.sweeps),
             "baseline": lambda: solver.baseline(num_scenes=S, seed=0, max_sweeps=a.sweeps)}
    res, wall = {}, {k: [] for k in calls}
    for i in range(a.warmup + a.solves):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = fn()
            torch.cuda.synchronize()
            if i >= a.warmup:
                wall[k].append(1e3 * (time.perf_counter() - t0))

    def stat(ms):
        ms = sorted(ms)
        return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}

    # ---- the launch alone: the env holds the scenes of seed 0 (baseline() ran last; the same scenes)
    env = solver.env
    start = res["solve0"].assignment
    out = torch.empty_like(start)
    J = torch.empty(S, dtype=torch.float64, device=dev)
    cov = torch.empty(S, dtype=torch.int32, device=dev)
    st = torch.empty(S, 4, dtype=torch.int32, device=dev)

    def time_launch(first):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for i in range(a.warmup + a.launches):
            j = i - a.warmup
            if j >= 0:
                ev[j][0].record()
            env.refine_assignments(first, stride=K, rows=S, max_sweeps=a.sweeps, out=out, J=J, covered=cov, stats=st)
            if j >= 0:
                ev[j][1].record()
        torch.cuda.synchronize()
        return stat([s.elapsed_time(e) for s, e in ev])

    refine_launch = time_launch(start)
    assert torch.equal(out, res["solve32"].assignment) and torch.equal(J, res["solve32"].J)
    baseline_launch = time_launch(None)
    assert torch.equal(out, res["baseline"].assignment) and torch.equal(J, res["baseline"].J)

    r0, r32, rb = res["solve0"], res["solve32"], res["baseline"]
    assert torch.equal(r32.decoded_J, r0.J)
    walls = {k: stat(v) for k, v in wall.items()}
    o = {"workload": f"{S} scenes x {N} x {M}, K = {K}, max_sweeps = {a.sweeps}", "device": torch.cuda.get_device_name(0),
         "policy": policy, "rounds": a.solves, "launches": a.launches,
         "wall_ms": walls, "refine_launch_ms": refine_launch, "baseline_launch_ms": baseline_launch,
         "refine_over_solve0": refine_launch["median"] / walls["solve0"]["median"],
         "solve32_minus_solve0_ms": walls["solve32"]["median"] - walls["solve0"]["median"],
         "mean_J_decoded": float(r0.J.mean()), "mean_J_refined": float(r32.J.mean()),
         "mean_J_baseline": float(rb.J.mean()),
         "refined_beats_baseline": float((r32.J > rb.J).double().mean()),
         "decoded_beats_baseline": float((r0.J > rb.J).double().mean()),
         "refine_mean_sweeps": float(r32.refine_stats[:, 0].double().mean()),
         "refine_max_sweeps": int(r32.refine_stats[:, 0].max()),
         "refine_mean_moves": float(r32.refine_stats[:, 1].double().mean()),
         "refine_converged": float(r32.refine_stats[:, 2].double().mean()),
         "baseline_mean_sweeps": float(rb.refine_stats[:, 0].double().mean()),
         "baseline_max_sweeps": int(rb.refine_stats[:, 0].max()),
         "baseline_converged": float(rb.refine_stats[:, 2].double().mean()),
         "unfinished": int((r0.best_replica < 0).sum())}
    print(json.dumps(o))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(o, indent=1) + "\n")


if __name__ == "__main__":
    main()
