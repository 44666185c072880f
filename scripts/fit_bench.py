#!/usr/bin/env python3
"""What the training driver (uavhip.fit.TrainingRun) costs beside the bare loop, and the
first learning curve of a policy it trained, in one process on one GPU at 4096 x 16 x 32, T = 64,
minibatch 4096:

  rate     --rounds alternating runs with diagnostics every iteration and with diagnostics off, each
           --warmup + --iterations iterations: env-steps/s of the timed iterations (host clock around
           them, ending in a device synchronise), ms per iteration, and the phase split -- rollout,
           update and diagnostics from HIP events on the launch stream; `drain` the host time of
           EpisodeStats.drain() (the iteration's last host sync: it waits for the diagnostics launches
           queued before it, so drain - diagnostics is the sync and the record copy); `files` the host
           time of progress.jsonl and the checkpoint writes
  curve    one run of --long iterations with the evaluation every --eval-every iterations on
           --eval-scenes fixed scenes: eval_mean_J beside the non-learned baseline's, the share of
           scenes where the greedy decode beats it, and the update diagnostics at those iterations

Prints one JSON line; --out also writes it (profiles/fit_run.json is a recorded run). bench.py
--full's e2e_iteration.minibatch_4096 is the bare loop the rate is read against.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "target-allocation-ppo-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(run, warmup, iterations):
    import torch
    for _ in range(warmup):
        run.step()
    for k in run.phase_ms:
        run.phase_ms[k] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    per_it = []
    for _ in range(iterations):
        per_it.append(run.step()["env_steps_per_s"])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"env_steps_per_s": iterations * run.T * run.E / dt, "ms_per_iteration": dt / iterations * 1e3,
            "per_iteration_env_steps_per_s": {"median": statistics.median(per_it), "min": min(per_it),
                                              "max": max(per_it)},
            "phase_ms": {k: v / iterations for k, v in run.phase_ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--minibatch", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--long", type=int, default=300, help="iterations of the learning-curve run (0: skip)")
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--eval-scenes", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from uavhip.fit import TrainingRun
    shape = dict(envs=a.envs, uavs=a.uavs, targets=a.targets, horizon=a.horizon, minibatch=a.minibatch, seed=a.seed)
    tmp = tempfile.mkdtemp(prefix="fit_bench_")
    res = {"device": torch.cuda.get_device_name(0), "shape": shape, "warmup": a.warmup, "iterations": a.iterations,
           "rate": {"diagnostics_every_1": [], "diagnostics_off": []}}
    try:
        for r in range(a.rounds):
            for name, every in (("diagnostics_every_1", 1), ("diagnostics_off", 0)):
                run = TrainingRun(out_dir=os.path.join(tmp, f"{name}_{r}"), diagnostics_every=every, **shape)
                res["rate"][name].append(timed(run, a.warmup, a.iterations))
                del run
                torch.cuda.empty_cache()
        on = statistics.median(x["ms_per_iteration"] for x in res["rate"]["diagnostics_every_1"])
        off = statistics.median(x["ms_per_iteration"] for x in res["rate"]["diagnostics_off"])
        res["diagnostics_share_of_iteration"] = (on - off) / on
        if a.long > 0:
            out = os.path.join(tmp, "long")
            run = TrainingRun(out_dir=out, eval_every=a.eval_every, eval_scenes=a.eval_scenes, **shape)
            t0 = time.perf_counter()
            summary = run.fit(a.long)
            keys = ("iteration", "env_steps", "eval_mean_J", "eval_mean_J_baseline", "eval_beats_baseline",
                    "mean_ep_reward", "mean_ep_J", "entropy", "approx_kl", "clip_frac", "explained_var", "loss_critic")
            with open(os.path.join(out, "progress.jsonl")) as fh:
                lines = [json.loads(x) for x in fh]
            res["curve"] = {"iterations": a.long, "eval_every": a.eval_every, "eval_scenes": a.eval_scenes,
                            "wall_s": time.perf_counter() - t0, "env_steps_per_s": summary["env_steps_per_s"],
                            "points": [{k: x.get(k) for k in keys} for x in lines
                                       if "eval_mean_J" in x or x["iteration"] == 1]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
