#!/usr/bin/env python3
"""What the optimum costs and what it says about the yardsticks (uavhip_solve_exact), in
one process on one GPU:

  launch     uavhip_solve_exact on --rows generated scenes of 16 x 32 (all rows in one workspace), by HIP
             events: median of --launches after --warmup; rows per second; uavhip_search_assignments'
             launch on the same rows, for scale
  kernels    the mean time of one k_exact_stage launch and of k_exact_backtrack, from torch's profiler over
             one call (None where the profiler does not see the kernels), and the stage time by
             difference: (the launch at M targets - the launch at 1 target) / (M - 1)
  cpu        the yardstick scripts/micro/exact_cpu.cpp (g++ -O2 -fopenmp, OMP_NUM_THREADS = --threads) on
             the first --cpu-scenes rows' tables read back from the device: its J must be the kernel's to
             1e-9, its seconds per scene give rows per second, and gpu_over_cpu is the ratio
  quality    on --scenes generated scenes, at omega = 0 (the config's) and omega = 0.5 (the tests' second):
             mean J of the optimum, of the baseline (best-response search), of the exchange search and of an
             UNTRAINED policy's greedy decode, each one's share of the optimum, and the share of scenes where
             each reaches it (J >= J* - 1e-12 max(1, |J*|))

Timings are recorded, not asserted. Prints one JSON line; --out also writes it (profiles/exact_bench.json
is a recorded run, --session names it).
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "target-allocation-ppo-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def cpu_yardstick(env, J, scenes, threads, omega):
    """Build and run scripts/micro/exact_cpu.cpp on the first `scenes` rows -> (seconds per scene, max |J - J_gpu|)."""
    import numpy as np
    N, M = env.N, env.M
    pd, pp, v, c = (getattr(env, k)[:scenes].cpu().numpy() for k in ("p_dmg", "p_pen", "tgt_value", "uav_cost"))
    with tempfile.TemporaryDirectory() as tmp:
        exe, tabs = os.path.join(tmp, "exact_cpu"), os.path.join(tmp, "tables.bin")
        subprocess.run(["g++", "-O2", "-fopenmp", "-o", exe, os.path.join(ROOT, "scripts", "micro", "exact_cpu.cpp")],
                       check=True)
        with open(tabs, "wb") as f:
            f.write(struct.pack("<iiid", N, M, scenes, omega))
            for s in range(scenes):
                f.write((pd[s] * pp[s][:, None]).astype("<f8").tobytes() + v[s].astype("<f8").tobytes() +
                        c[s].astype("<f8").tobytes())
        out = subprocess.run([exe, tabs], check=True, capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=str(threads))).stdout.split("\n")
    Jc = np.array([float(l.split()[1]) for l in out if l.startswith("J ")])
    sec = float(next(l for l in out if l.startswith("seconds_per_scene")).split()[1])
    err = float(np.abs(Jc - J[:scenes].cpu().numpy()).max())
    assert err <= 1e-9, (Jc, J[:scenes])
    return sec, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-scenes", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--session", default=None, help="a name for the recorded run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import copy

    import torch
    from uavhip import AllocationSolver, _lib
    from uavhip.config import cfg
    from uavhip.policy import TransformerActorCritic
    from uavhip.vec_env import VecUAVEnv
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    R, N, M = a.rows, a.uavs, a.targets
    row_bytes = int(_lib.LIB.uavhip_exact_workspace_bytes(N, M, 1))

    def timed(calls, launches, warmup):
        """Median / min / max ms of each call, the calls alternating."""
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
              for k in calls}
        for i in range(warmup + launches):
            for k, fn in calls.items():
                if i >= warmup:
                    ev[k][i - warmup][0].record()
                fn()
                if i >= warmup:
                    ev[k][i - warmup][1].record()
        torch.cuda.synchronize()
        out = {}
        for k, v in ev.items():
            ms = sorted(s.elapsed_time(e) for s, e in v)
            out[k] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}
        return out

    def bufs(S, n_stats):
        return dict(out=torch.empty(S, N, dtype=torch.int32, device=dev), J=torch.empty(S, dtype=torch.float64, device=dev),
                    covered=torch.empty(S, dtype=torch.int32, device=dev),
                    stats=torch.empty(S, n_stats, dtype=torch.int32, device=dev))

    # ---------------------------------------------------------------- launch times
    env = VecUAVEnv(R, N, M, device=dev, seed=a.seed, full_reset_period=0, scene_buffers=1)
    env.generate_scenes()
    be, bs = bufs(R, 2), bufs(R, 6)
    big = R * row_bytes
    ms = timed({"exact": lambda: env.exact_assignments(None, max_workspace_bytes=big, **be),
                "search": lambda: env.search_assignments(None, **bs)}, a.launches, a.warmup)
    one = VecUAVEnv(R, N, 1, device=dev, seed=a.seed, full_reset_period=0, scene_buffers=1)
    one.generate_scenes()
    b1 = bufs(R, 2)
    ms1 = timed({"exact": lambda: one.exact_assignments(None, **b1)}, 5, 2)["exact"]
    kernels = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            env.exact_assignments(None, max_workspace_bytes=big, **be)
            torch.cuda.synchronize()
        seen = {}
        for e in prof.events():
            for name in ("k_exact_prepare", "k_exact_stage", "k_exact_backtrack"):
                if name in e.name:
                    seen.setdefault(name, []).append(e.device_time if hasattr(e, "device_time") else e.cuda_time)
        if seen:
            kernels = {k: {"launches": len(v), "mean_ms": sum(v) / len(v) / 1e3} for k, v in seen.items()}
    except Exception as ex:  # the profiler is a convenience here; the differential below does not need it
        kernels = {"error": repr(ex)}
    cpu_s, cpu_err = cpu_yardstick(env, be["J"], min(a.cpu_scenes, R), a.threads, float(cfg.COST_WEIGHT_OMEGA))
    gpu_rows_per_s = R / (ms["exact"]["median"] * 1e-3)

    # ---------------------------------------------------------------- what the yardsticks reach
    quality = {}
    torch.manual_seed(a.seed)
    net = TransformerActorCritic().to(dev)
    for omega in (0.0, 0.5):
        c = copy.copy(cfg)
        c.COST_WEIGHT_OMEGA = omega
        solver = AllocationSolver(net, N, M, config=c, samples=1)
        args = dict(num_scenes=a.scenes, seed=a.seed)
        best = solver.optimum(**args).J
        runs = {"baseline": solver.baseline(**args).J, "exchange_search": solver.baseline(exchanges=32, **args).J,
                "untrained_decode": solver.solve(**args).J}
        tol = 1e-12 * best.abs().clamp(min=1.0)
        q = {"mean_J_optimal": float(best.mean())}
        for k, J in runs.items():
            assert bool((J <= best + tol).all()), k
            q[k] = {"mean_J": float(J.mean()), "over_optimal": float(J.mean() / best.mean()),
                    "is_optimal": float((J >= best - tol).double().mean()),
                    "worst_row_over_optimal": float((J / best).min())}
        quality[f"omega_{omega}"] = q

    o = {"workload": f"{R} rows x {N} x {M} in one workspace of {big} bytes, unconstrained, generated scenes",
         "session": a.session, "device": torch.cuda.get_device_name(0), "launches": a.launches, "warmup": a.warmup,
         "workspace_bytes_per_row": row_bytes, "launch_ms": ms, "rows_per_s": gpu_rows_per_s,
         "search_rows_per_s": R / (ms["search"]["median"] * 1e-3),
         "launch_ms_at_one_target": ms1, "stage_ms_by_difference": (ms["exact"]["median"] - ms1["median"]) / (M - 1),
         "kernels_by_profiler": kernels,
         "cpu": {"program": "scripts/micro/exact_cpu.cpp, g++ -O2 -fopenmp", "threads": a.threads,
                 "scenes": min(a.cpu_scenes, R), "seconds_per_scene": cpu_s, "rows_per_s": 1.0 / cpu_s,
                 "max_abs_J_difference_to_the_kernel": cpu_err},
         "gpu_over_cpu": gpu_rows_per_s * cpu_s, "scenes": a.scenes, "quality": quality}
    print(json.dumps(o))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(o, indent=1) + "\n")


if __name__ == "__main__":
    main()
