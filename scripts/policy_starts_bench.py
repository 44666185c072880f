#!/usr/bin/env python3
"""Policy starts against random starts at equal R (uavhip_search_multistart_from), in one
process on one GPU:

  launch     --rows generated scenes of 16 x 32 decoded K = R = 16 times by the policy, caps 32 / 32:
             uavhip_search_multistart_from with R0 in --given of the decoded replicas as given starts,
             beside uavhip_search_multistart at the same R on the same rows (from decoded replica 0), all
             alternating, by HIP events: median of --launches after --warmup, min and max; per R0 the ratio
             to the existing launch and whether its median lies inside that launch's min-max; the mean
             sweeps, moves and exchanges per given replica beside those of the random replicas, read from
             the per-replica counters the kernel leaves in the workspace
             (J [W] f64 | ids [W][N] i32 | covered [W] i32 | counters [W][8] i32, W = rows x R); and the
             number of distinct starts among a scene's K decoded replicas
  quality    on optimum(num_scenes=--scenes, seed)'s scenes at omega = 0 and omega = 0.5, R = 16: mean J, its
             share of the optimum's mean J, the scenes that reach the optimum (J >= J* - 1e-12 max(1, |J*|))
             and the worst scene's share, for 16 random starts (baseline(exchanges=32, restarts=16)), the
             best decoded replica plus 15 random (solve(restarts=16)), 8 policy plus 8 random and 16 policy
             (solve(restarts=16, starts="replicas") at samples = 8 and 16); for the two last also the share
             of scenes a policy start wins and the distinct starts per scene

The policy is the seeded initial one (torch.manual_seed(--seed)) unless --checkpoint is given; the JSON
says which. Timings are recorded, not asserted. Prints one JSON line; --out also writes it
(profiles/policy_starts_bench.json is a recorded run, --session names it).
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
    ap.add_argument("--restarts", type=int, default=16, help="R, and the K of the launch leg's decode")
    ap.add_argument("--given", type=int, nargs="+", default=[1, 8, 16], help="the R0 of the launch leg")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--checkpoint", default=None, help="a torch.save(policy.state_dict()) file instead of the initial policy")
    ap.add_argument("--session", default=None, help="a name for the recorded run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import copy

    import numpy as np
    import torch
    from uavhip import AllocationSolver
    from uavhip.checkpoint import load_checkpoint
    from uavhip.config import cfg
    from uavhip.policy import TransformerActorCritic
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    S, N, M, R = a.rows, a.uavs, a.targets, a.restarts
    torch.manual_seed(a.seed)
    net = TransformerActorCritic().to(dev)
    if a.checkpoint:
        load_checkpoint(net, a.checkpoint)

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

    def bufs(rows):
        return dict(out=torch.empty(rows, N, dtype=torch.int32, device=dev),
                    J=torch.empty(rows, dtype=torch.float64, device=dev),
                    covered=torch.empty(rows, dtype=torch.int32, device=dev),
                    stats=torch.empty(rows, 10, dtype=torch.int32, device=dev))

    def replica_counters(env, rows):
        """The per-replica counters of the last call, from its workspace: [rows, R, 8] on the host."""
        W = rows * R
        off = 8 * W + 4 * W * N + 4 * W
        return env._multistart_ws[off:off + 32 * W].view(torch.int32).view(rows, R, 8).cpu().double()

    def counters(c):
        return {"mean_sweeps": float(c[..., 0].mean()), "mean_moves": float(c[..., 1].mean()),
                "mean_exchanges": float(c[..., 4].mean()), "max_sweeps": float(c[..., 0].max()),
                "share_not_converged": float(1.0 - (c[..., 2] * c[..., 5]).mean())}

    def distinct_starts(given):
        """The mean number of distinct assignments among a scene's K given starts."""
        g = given.cpu().numpy()
        return float(np.mean([len({row.tobytes() for row in scene}) for scene in g]))

    # ---------------------------------------------------------------- launch times at 16 x 32, K = R decoded replicas
    solver = AllocationSolver(net, N, M, samples=R)
    solver.solve(num_scenes=S, seed=a.seed)
    env = solver.env
    given = env.assigned_target_ids().to(torch.int32).view(S, R, N).contiguous()
    first = given[:, 0].contiguous()
    rows = dict(seed=a.seed, stride=R, rows=S, restarts=R)
    bm = {k: bufs(S) for k in ["multistart"] + [f"from_R0_{g}" for g in a.given]}
    starts = {g: given[:, :g].contiguous() for g in a.given}
    calls = {"multistart": lambda: env.search_assignments_multistart(first, **rows, **bm["multistart"])}
    for g in a.given:
        calls[f"from_R0_{g}"] = (lambda g=g: env.search_assignments_multistart(None, starts=starts[g], **rows,
                                                                                **bm[f"from_R0_{g}"]))
    ms = timed(calls)
    ref = ms["multistart"]
    launch = {}
    for k, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        c = replica_counters(env, S)
        g = 1 if k == "multistart" else int(k.rsplit("_", 1)[1])
        o = dict(ms[k], mean_J=float(bm[k]["J"].mean()), over_multistart=ms[k]["median"] / ref["median"],
                 median_inside_multistart_min_max=bool(ref["min"] <= ms[k]["median"] <= ref["max"]),
                 given_wins=float((bm[k]["stats"][:, 8] < g).double().mean()), given_replicas=counters(c[:, :g]))
        if g < R:
            o["random_replicas"] = counters(c[:, g:])
        launch[k] = o
    if 1 in a.given:  # one given start is the existing call
        assert all(torch.equal(bm["multistart"][k], bm["from_R0_1"][k]) for k in bm["multistart"])
    launch["distinct_starts_per_scene"] = distinct_starts(given)
    del solver, env

    # ---------------------------------------------------------------- what the starts reach, against the optimum
    quality = {}
    for omega in (0.0, 0.5):
        c = copy.copy(cfg)
        c.COST_WEIGHT_OMEGA = omega
        args = dict(num_scenes=a.scenes, seed=a.seed)
        polish = dict(refine=32, exchanges=32, restarts=R)
        full = AllocationSolver(net, N, M, config=c, samples=R)
        half = AllocationSolver(net, N, M, config=c, samples=R // 2)
        best = full.optimum(**args).J
        tol = 1e-12 * best.abs().clamp(min=1.0)
        q = {"mean_J_optimal": float(best.mean())}
        runs = {f"random_{R}": full.baseline(exchanges=32, restarts=R, **args),
                f"best_replica_plus_{R - 1}_random": full.solve(**polish, **args)}
        half_run = half.solve(starts="replicas", **polish, **args)
        half_distinct = distinct_starts(half.env.assigned_target_ids().view(a.scenes, R // 2, N))
        runs[f"policy_{R // 2}_plus_{R - R // 2}_random"] = half_run
        runs[f"policy_{R}"] = full.solve(starts="replicas", **polish, **args)
        full_distinct = distinct_starts(full.env.assigned_target_ids().view(a.scenes, R, N))
        for k, r in runs.items():
            J = r.J
            assert bool((J <= best + tol).all()), k
            q[k] = {"mean_J": float(J.mean()), "over_optimal": float(J.mean() / best.mean()),
                    "is_optimal": float((J >= best - tol).double().mean()), "scenes_optimal": int((J >= best - tol).sum()),
                    "worst_row_over_optimal": float((J / best).min())}
        rnd = runs[f"random_{R}"].J
        for k, K, d in ((f"policy_{R // 2}_plus_{R - R // 2}_random", R // 2, half_distinct), (f"policy_{R}", R, full_distinct)):
            r = runs[k]
            q[k].update(policy_start_wins=float((r.refine_stats[:, 8] < K).double().mean()),
                        beats_random=float((r.J > rnd).double().mean()), below_random=float((r.J < rnd).double().mean()),
                        distinct_starts_per_scene=d, mean_J_decoded_best=float(r.decoded_J.mean()),
                        unfinished_scenes=int((r.best_replica < 0).sum()))
        quality[f"omega_{omega}"] = q
        del full, half

    o = {"workload": f"{S} rows x {N} x {M}, unconstrained, generated scenes, K = R = {R} decoded replicas, caps 32 / 32",
         "policy": os.path.basename(a.checkpoint) if a.checkpoint else f"the initial policy of torch.manual_seed({a.seed})",
         "session": a.session, "device": torch.cuda.get_device_name(0), "launches": a.launches, "warmup": a.warmup,
         "seed": a.seed, "R": R, "launch_ms": launch, "scenes": a.scenes, "quality": quality}
    print(json.dumps(o))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(o, indent=1) + "\n")


if __name__ == "__main__":
    main()
