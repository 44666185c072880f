#!/usr/bin/env python3
"""What the exchange-move local search (uavhip_search_assignments) costs and buys beside
the plain best-response search (uavhip_refine_assignments, 9b), in one process on one GPU at 4096
scenes x 16 x 32 with K = 8 replicas:

  launch   the k_search launch (max_exchanges / max_sweeps = 32 / 32) and the k_refine launch
           (max_sweeps = 32) alone by HIP events, the two ALTERNATING on the same inputs: from the
           best-of-K assignment of a solve at env_stride = K, and from the empty assignment; median
           of --launches after --warmup, and the ratio of the medians
  wall     host clock around solve(refine=0), solve(refine=32) and solve(refine=32, exchanges=32)
           (ending in a device synchronise), alternating, median and range of --solves rounds
  J        mean J of the baseline and of the refined allocations with and without exchanges, mean and
           maximum exchanges per scene, the share of scenes the exchanges improve, and the share left
           with scan_clean = 0 (the cap of 32 exchanges reached)

The policy is --checkpoint, or else the seeded initial policy (torch.manual_seed(0)): UNTRAINED, so
its J figures say nothing about a trained policy. Timings are recorded, not asserted. Prints one JSON
line; --out also writes it (profiles/search_bench.json is a recorded run).
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
    ap.add_argument("--exchanges", type=int, default=32)
    ap.add_argument("--solves", type=int, default=5, help="timed rounds of the three solves")
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
    S, N, M, K, R, X = a.scenes, a.uavs, a.targets, a.samples, a.sweeps, a.exchanges
    solver = AllocationSolver(net, N, M, samples=K)
    calls = {"solve0": lambda: solver.solve(num_scenes=S, seed=0),
             "solve_refine": lambda: solver.solve(num_scenes=S, seed=0, refine=R),
             "solve_exchange": lambda: solver.solve(num_scenes=S, seed=0, refine=R, exchanges=X)}
    res, wall = {}, {k: [] for k in calls}
    for i in range(a.warmup + a.solves):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = fn()
            torch.cuda.synchronize()
            if i >= a.warmup:
                wall[k].append(1e3 * (time.perf_counter() - t0))
    base = solver.baseline(num_scenes=S, seed=0, max_sweeps=R)
    base_x = solver.baseline(num_scenes=S, seed=0, max_sweeps=R, exchanges=X)

    def stat(ms):
        ms = sorted(ms)
        return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}

    # ---- the launches alone: the env holds the scenes of seed 0 (the baselines ran last; the same scenes)
    env = solver.env
    start = res["solve0"].assignment
    out = torch.empty_like(start)
    J = torch.empty(S, dtype=torch.float64, device=dev)
    cov = torch.empty(S, dtype=torch.int32, device=dev)
    st4 = torch.empty(S, 4, dtype=torch.int32, device=dev)
    st6 = torch.empty(S, 6, dtype=torch.int32, device=dev)

    def refine(first):
        env.refine_assignments(first, stride=K, rows=S, max_sweeps=R, out=out, J=J, covered=cov, stats=st4)

    def search(first):
        env.search_assignments(first, stride=K, rows=S, max_exchanges=X, max_sweeps=R, out=out, J=J, covered=cov,
                               stats=st6)

    def time_launches(first):
        """(k_refine, k_search) launch times, the two alternating."""
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(a.launches)] for k in ("refine", "search")}
        for i in range(a.warmup + a.launches):
            j = i - a.warmup
            for k, fn in (("refine", refine), ("search", search)):
                if j >= 0:
                    ev[k][j][0].record()
                fn(first)
                if j >= 0:
                    ev[k][j][1].record()
        torch.cuda.synchronize()
        return {k: stat([s.elapsed_time(e) for s, e in v]) for k, v in ev.items()}

    polish = time_launches(start)
    assert torch.equal(out, res["solve_exchange"].assignment) and torch.equal(J, res["solve_exchange"].J)
    empty = time_launches(None)
    assert torch.equal(out, base_x.assignment) and torch.equal(J, base_x.J)

    r0, rr, rx = res["solve0"], res["solve_refine"], res["solve_exchange"]
    assert torch.equal(rr.decoded_J, r0.J) and torch.equal(rx.decoded_J, r0.J)
    walls = {k: stat(v) for k, v in wall.items()}

    def counters(r, plain):
        s = r.refine_stats
        return {"mean_exchanges": float(s[:, 4].double().mean()), "max_exchanges": int(s[:, 4].max()),
                "mean_sweeps": float(s[:, 0].double().mean()), "max_sweeps": int(s[:, 0].max()),
                "mean_moves": float(s[:, 1].double().mean()),
                "scenes_improved": float((r.J > plain.J).double().mean()),
                "scenes_worse": float((r.J < plain.J).double().mean()),
                "scan_not_clean": float((s[:, 5] == 0).double().mean()),
                "phase_not_converged": float((s[:, 2] == 0).double().mean())}

    o = {"workload": f"{S} scenes x {N} x {M}, K = {K}, max_sweeps = {R}, max_exchanges = {X}",
         "device": torch.cuda.get_device_name(0), "policy": policy, "rounds": a.solves, "launches": a.launches,
         "launch_ms_from_best_of_K": polish, "launch_ms_from_empty": empty,
         "search_over_refine_from_best_of_K": polish["search"]["median"] / polish["refine"]["median"],
         "search_over_refine_from_empty": empty["search"]["median"] / empty["refine"]["median"],
         "wall_ms": walls,
         "search_launch_over_solve0": polish["search"]["median"] / walls["solve0"]["median"],
         "solve_exchange_minus_solve_refine_ms": walls["solve_exchange"]["median"] - walls["solve_refine"]["median"],
         "mean_J_decoded": float(r0.J.mean()), "mean_J_refined": float(rr.J.mean()),
         "mean_J_refined_exchange": float(rx.J.mean()), "mean_J_baseline": float(base.J.mean()),
         "mean_J_baseline_exchange": float(base_x.J.mean()),
         "refined": counters(rx, rr), "baseline": counters(base_x, base),
         "refined_exchange_beats_baseline": float((rx.J > base.J).double().mean()),
         "refined_exchange_beats_baseline_exchange": float((rx.J > base_x.J).double().mean()),
         "unfinished": int((r0.best_replica < 0).sum())}
    print(json.dumps(o))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(o, indent=1) + "\n")


if __name__ == "__main__":
    main()
