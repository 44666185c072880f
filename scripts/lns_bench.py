#!/usr/bin/env python3
"""What the exact neighbourhood search costs and what it buys (uavhip_solve_exact_free,
uavhip_neighbourhood_pick, VecUAVEnv.lns_assignments), in one process on one GPU:

  launch   one uavhip_solve_exact_free launch on --rows generated scenes of 64 x 128 from the exchange
           search's result, a random max_free-set of each row free, for max_free in --free, all
           alternating, by HIP events: median of --launches after --warmup; and the maximisation steps
           per second (3^max_free x M x rows a launch) beside uavhip_solve_exact's recorded rate
  quality  on optimum(num_scenes=--scenes, seed)'s scenes of 16 x 32 at omega = 0 and omega = 0.5, from
           baseline(exchanges=32): the share of the optimum's mean J and the share of scenes optimal after
           --rounds rounds of LNS with K in --lns-free, both modes; the time of the whole LNS call; and
           beside each the multi-start search (R in --restarts) whose launch time is closest to it
  large    at 64 x 128 on --rows generated scenes, where no optimum can be had: mean J of the exchange
           search, of multi-start at every R of --restarts, and of LNS from the exchange search's result at
           K = 12; the share of scenes where LNS ends strictly above the multi-start of the nearest time,
           and the other way round

Timings are recorded, not asserted. --legs chooses the legs; a leg's result is merged into --out
(profiles/lns_bench.json is a recorded run, --session names it). Prints one JSON line per leg.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "target-allocation-ppo-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

EXACT_RECORDED_STEPS_PER_S = 0.18e12  # uavhip_solve_exact, 256 rows x 16 x 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["launch", "quality", "large"], choices=("launch", "quality", "large"))
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--free", type=int, nargs="+", default=[8, 10, 12, 14, 16])
    ap.add_argument("--lns-free", type=int, nargs="+", default=[8, 12])
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--restarts", type=int, nargs="+", default=[1, 4, 16, 64, 256, 1024])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
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
            print(f"  pass {i + 1} of {a.warmup + a.launches}", file=sys.stderr, flush=True)
        out = {}
        for k, v in ev.items():
            ms = sorted(s.elapsed_time(e) for s, e in v)
            out[k] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}
        return out

    def nearest(ms, target):
        """The key of `ms` whose median is closest to `target` ms."""
        return min(ms, key=lambda k: abs(ms[k]["median"] - target))

    def record(leg, result):
        o = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                o = json.load(f)
        o.update({"session": a.session, "device": torch.cuda.get_device_name(0), "launches": a.launches,
                  "warmup": a.warmup, "seed": a.seed, leg: result})
        print(json.dumps({leg: result}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(o, indent=1) + "\n")

    def lns_leg(env, start, J_start, free, modes, stride, rows, **con):
        """Per (K, mode): the whole lns_assignments call timed beside every multi-start R, its J."""
        calls, res = {}, {}
        for K in free:
            for mode in modes:
                calls[f"lns_K{K}_{mode}"] = (lambda K=K, mode=mode: res.__setitem__(
                    (K, mode), env.lns_assignments(start, rounds=a.rounds, free=K, mode=mode, seed=a.seed, stride=stride,
                                                   rows=rows, **con)))
        for R in a.restarts:
            calls[f"multistart_R{R}"] = (lambda R=R: res.__setitem__(
                R, env.search_assignments_multistart(None, restarts=R, seed=a.seed, stride=stride, rows=rows)))
        ms = timed(calls)
        return ms, res

    # ---------------------------------------------------------------- one launch at 64 x 128
    if "launch" in a.legs:
        S, N, M = a.rows, 64, 128
        env = VecUAVEnv(S, N, M, device=dev, seed=a.seed, full_reset_period=0, scene_buffers=1)
        env.generate_scenes()
        start, J0 = env.search_assignments(None)[:2]
        g = torch.Generator().manual_seed(a.seed)
        order = torch.stack([torch.randperm(N, generator=g) for _ in range(S)])
        out = {}
        for K in a.free:  # one max_free at a time: the alternation is over launches of the same table size
            fixed = torch.ones(S, N, dtype=torch.uint8)
            fixed.scatter_(1, order[:, :K], 0)
            fixed = fixed.to(dev)
            res = {}
            ms = timed({"exact_free": lambda: res.__setitem__(0, env.exact_free_assignments(start, max_free=K, fixed=fixed))})
            steps = 3.0 ** K * M * S
            J = res[0][1]
            out[f"max_free_{K}"] = dict(ms["exact_free"], steps_per_s=steps / (ms["exact_free"]["median"] * 1e-3),
                                        over_solve_exact_rate=steps / (ms["exact_free"]["median"] * 1e-3) / EXACT_RECORDED_STEPS_PER_S,
                                        workspace_bytes=int(env._exact_free_ws.numel()),
                                        mean_J_in=float(J0.mean()), mean_J_out=float(J.mean()),
                                        rows_improved=float((J > J0).double().mean()),
                                        rows_below=int((J < J0 - 1e-12 * J0.abs().clamp(min=1.0)).sum()))
            del env._exact_free_ws
        record("launch", {"workload": f"{S} rows x {N} x {M}, from the exchange search, a random max_free-set free", **out})
        del env

    # ---------------------------------------------------------------- what LNS reaches where the optimum is known
    if "quality" in a.legs:
        N, M = 16, 32
        torch.manual_seed(a.seed)
        net = TransformerActorCritic().to(dev)
        quality = {}
        for omega in (0.0, 0.5):
            c = copy.copy(cfg)
            c.COST_WEIGHT_OMEGA = omega
            solver = AllocationSolver(net, N, M, config=c, samples=1)
            args = dict(num_scenes=a.scenes, seed=a.seed)
            best = solver.optimum(**args).J
            tol = 1e-12 * best.abs().clamp(min=1.0)
            base = solver.baseline(exchanges=32, **args)
            ms, res = lns_leg(solver.env, base.assignment, base.J, a.lns_free, ("random", "targets"), 1, a.scenes)

            def reach(J):
                assert bool((J <= best + tol).all())
                return {"mean_J": float(J.mean()), "over_optimal": float(J.mean() / best.mean()),
                        "is_optimal": float((J >= best - tol).double().mean())}
            q = {"mean_J_optimal": float(best.mean()), "exchange_search": reach(base.J)}
            for R in a.restarts:
                q[f"multistart_R{R}"] = dict(reach(res[R][1]), ms=ms[f"multistart_R{R}"])
            for K in a.lns_free:
                for mode in ("random", "targets"):
                    key = f"lns_K{K}_{mode}"
                    J = res[(K, mode)][1]
                    assert bool((J >= base.J).all())
                    near = nearest({k: v for k, v in ms.items() if k.startswith("multistart")}, ms[key]["median"])
                    q[key] = dict(reach(J), ms=ms[key], rows_improved=float((J > base.J).double().mean()),
                                  mean_improving_rounds=float(res[(K, mode)][3].double().mean()),
                                  multistart_at_nearest_time=near)
            quality[f"omega_{omega}"] = q
            del solver
        record("quality", {"workload": f"{a.scenes} generated scenes x {N} x {M}, {a.rounds} rounds from "
                                       f"baseline(exchanges=32)", **quality})

    # ---------------------------------------------------------------- the largest shape: no optimum there
    if "large" in a.legs:
        S, N, M = a.rows, 64, 128
        env = VecUAVEnv(S, N, M, device=dev, seed=a.seed, full_reset_period=0, scene_buffers=1)
        env.generate_scenes()
        start, J0 = env.search_assignments(None)[:2]
        ms, res = lns_leg(env, start, J0, [12], ("random", "targets"), 1, S)
        large = {"exchange_search": {"mean_J": float(J0.mean())}}
        for R in a.restarts:
            large[f"multistart_R{R}"] = {"mean_J": float(res[R][1].mean()), "ms": ms[f"multistart_R{R}"]}
        for mode in ("random", "targets"):
            key = f"lns_K12_{mode}"
            J = res[(12, mode)][1]
            assert bool((J >= J0).all())
            near = nearest({k: v for k, v in ms.items() if k.startswith("multistart")}, ms[key]["median"])
            Jm = res[int(near.split("R")[1])][1]
            large[key] = {"mean_J": float(J.mean()), "ms": ms[key], "rows_improved": float((J > J0).double().mean()),
                          "mean_improving_rounds": float(res[(12, mode)][3].double().mean()),
                          "multistart_at_nearest_time": near, "lns_above_it": float((J > Jm).double().mean()),
                          "it_above_lns": float((Jm > J).double().mean())}
        record("large", {"workload": f"{S} generated scenes x {N} x {M}, {a.rounds} rounds from the exchange search",
                         **large})


if __name__ == "__main__":
    main()
