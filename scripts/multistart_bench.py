#!/usr/bin/env python3
"""What R restarts of the exchange search cost and what they buy (uavhip_search_multistart, DESIGN.md
9j), in one process on one GPU:

  launch     uavhip_search_multistart on --rows generated scenes of 16 x 32 from the empty start, caps
             32 / 32, for R in --restarts, beside uavhip_search_assignments on the same rows, all
             alternating, by HIP events: median of --launches after --warmup; per R the ratio to R x the
             single launch, and the mean sweeps and exchanges per replica (replica 0 apart from the
             random starts), read from the per-replica counters the kernel leaves in the workspace
             (J [W] f64 | ids [W][N] i32 | covered [W] i32 | counters [W][8] i32, W = rows x R)
  quality    on optimum(num_scenes=--scenes, seed)'s scenes at omega = 0 and omega = 0.5: per R the mean J
             of baseline(exchanges=32, restarts=R), its share of the optimum's mean J, the share of scenes
             where it reaches the optimum (J >= J* - 1e-12 max(1, |J*|)) and the worst scene's share
  large      one leg at --rows x 64 x 128, where no optimum can be had: launch time and mean J for R = 1
             and R = 16

Timings are recorded, not asserted. Prints one JSON line; --out also writes it
(profiles/multistart_bench.json is a recorded run, --session names it).
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
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--restarts", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--session", default=None, help="a name for the recorded run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import copy

    import torch
    from uavhip import AllocationSolver
    from uavhip.config import cfg
    from uavhip.policy import TransformerActorCritic
    from uavhip.vec_env import VecUAVEnv
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    S, N, M = a.rows, a.uavs, a.targets

    def timed(calls):
        """Median / min / max ms of each call, the calls alternating."""
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(a.launches)] for k in calls}
        for i in range(a.warmup + a.launches):
            for k, fn in calls.items():
                if i >= a.warmup:
                    ev[k][i - a.warmup][0].record()
                fn()
                if i >= a.warmup:
                    ev[k][i - a.warmup][1].record()
        torch.cuda.synchronize()
        out = {}
        for k, v in ev.items():
            ms = sorted(s.elapsed_time(e) for s, e in v)
            out[k] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}
        return out

    def bufs(rows, n, n_stats):
        return dict(out=torch.empty(rows, n, dtype=torch.int32, device=dev),
                    J=torch.empty(rows, dtype=torch.float64, device=dev),
                    covered=torch.empty(rows, dtype=torch.int32, device=dev),
                    stats=torch.empty(rows, n_stats, dtype=torch.int32, device=dev))

    def replica_counters(env, rows, n, R):
        """The per-replica counters of the last call, from its workspace: [rows, R, 8] on the host."""
        W = rows * R
        off = 8 * W + 4 * W * n + 4 * W
        return env._multistart_ws[off:off + 32 * W].view(torch.int32).view(rows, R, 8).cpu().double()

    def launch_leg(env, rows, n, restarts):
        bs = bufs(rows, n, 6)
        bm = {R: bufs(rows, n, 10) for R in restarts}
        calls = {"search": lambda: env.search_assignments(None, **bs)}
        for R in restarts:
            calls[f"multistart_R{R}"] = (lambda R=R: env.search_assignments_multistart(None, restarts=R, seed=a.seed,
                                                                                       **bm[R]))
        ms = timed(calls)
        single = ms["search"]["median"]
        out = {"search": dict(ms["search"], mean_J=float(bs["J"].mean()),
                              mean_sweeps=float(bs["stats"][:, 0].double().mean()),
                              mean_exchanges=float(bs["stats"][:, 4].double().mean()))}
        for R in restarts:
            env.search_assignments_multistart(None, restarts=R, seed=a.seed, **bm[R])
            torch.cuda.synchronize()
            c = replica_counters(env, rows, n, R)
            o = dict(ms[f"multistart_R{R}"], mean_J=float(bm[R]["J"].mean()),
                     over_R_single_launches=ms[f"multistart_R{R}"]["median"] / (R * single),
                     rows_improved=float((bm[R]["stats"][:, 9] > 0).double().mean()),
                     replica0={"mean_sweeps": float(c[:, 0, 0].mean()), "mean_exchanges": float(c[:, 0, 4].mean())})
            if R > 1:
                o["random_starts"] = {"mean_sweeps": float(c[:, 1:, 0].mean()), "mean_moves": float(c[:, 1:, 1].mean()),
                                      "mean_exchanges": float(c[:, 1:, 4].mean()),
                                      "max_sweeps": float(c[:, 1:, 0].max()),
                                      "share_not_converged": float(1.0 - (c[:, 1:, 2] * c[:, 1:, 5]).mean())}
            out[f"multistart_R{R}"] = o
        return out

    # ---------------------------------------------------------------- launch times at 16 x 32
    env = VecUAVEnv(S, N, M, device=dev, seed=a.seed, full_reset_period=0, scene_buffers=1)
    env.generate_scenes()
    launch = launch_leg(env, S, N, a.restarts)
    del env

    # ---------------------------------------------------------------- what the restarts reach
    quality = {}
    torch.manual_seed(a.seed)
    net = TransformerActorCritic().to(dev)
    for omega in (0.0, 0.5):
        c = copy.copy(cfg)
        c.COST_WEIGHT_OMEGA = omega
        solver = AllocationSolver(net, N, M, config=c, samples=1)
        args = dict(num_scenes=a.scenes, seed=a.seed)
        best = solver.optimum(**args).J
        tol = 1e-12 * best.abs().clamp(min=1.0)
        q = {"mean_J_optimal": float(best.mean())}
        runs = {"exchange_search": solver.baseline(exchanges=32, **args).J}
        for R in a.restarts:
            runs[f"multistart_R{R}"] = solver.baseline(exchanges=32, restarts=R, **args).J
        for k, J in runs.items():
            assert bool((J <= best + tol).all()), k
            q[k] = {"mean_J": float(J.mean()), "over_optimal": float(J.mean() / best.mean()),
                    "is_optimal": float((J >= best - tol).double().mean()), "scenes_optimal": int((J >= best - tol).sum()),
                    "worst_row_over_optimal": float((J / best).min())}
        if 1 in a.restarts:  # one replica is the exchange search itself
            assert torch.equal(runs["exchange_search"], runs["multistart_R1"])
        quality[f"omega_{omega}"] = q
        del solver

    # ---------------------------------------------------------------- the largest shape: no optimum there
    big = VecUAVEnv(S, 64, 128, device=dev, seed=a.seed, full_reset_period=0, scene_buffers=1)
    big.generate_scenes()
    large = launch_leg(big, S, 64, [1, 16])

    o = {"workload": f"{S} rows x {N} x {M}, unconstrained, generated scenes, the empty start, caps 32 / 32",
         "session": a.session, "device": torch.cuda.get_device_name(0), "launches": a.launches, "warmup": a.warmup,
         "seed": a.seed, "launch_ms": launch, "scenes": a.scenes, "quality": quality,
         "large": {"workload": f"{S} rows x 64 x 128", "launch_ms": large}}
    print(json.dumps(o))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(o, indent=1) + "\n")


if __name__ == "__main__":
    main()
