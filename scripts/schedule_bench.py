#!/usr/bin/env python3
"""What reading the PPO step's scheduled hyper-parameters from device memory costs
(uavhip_ppo_step_hyper), and the first learning curves with lr / entropy schedules
(uavhip.fit), on one GPU at 4096 x 16 x 32. Everything is recorded, nothing asserted.

  step     the optimizer step at minibatch 4096 and 64 in three variants: another build of the library
           given with --parent-lib (the commit before the entry point; loaded in a child process through
           UAVHIP_LIB), this build through uavhip_ppo_step (by value) and this build through
           uavhip_ppo_step_hyper (after set_hyper). One sample is a replay of a captured graph of
           --graph-steps minibatch steps between two HIP events, divided by the step count; a figure is
           the median of --reps samples after --warmup. The variants alternate: each of --rounds rounds
           starts one child per build, and the child of this build alternates by value / hyper sample by
           sample (the child of the other build alternates two by-value trainers, so every figure is taken
           with a second trainer's replays in between). The yardstick for "the same" is the min - max of
           the parent build's medians over the rounds.
  learn    --iterations TrainingRun iterations each of: constant; linear lr to 0.1; linear lr to 0.1
           plus linear entropy decay to 0 -- eval_mean_J of the greedy decode every --eval-every
           iterations beside the baseline. With --init-iterations > 0 also the DAgger recipe of
           scripts/dagger_bench.py (ImitationRun source="dagger") and, from its checkpoint, constant
           against lr_warmup 5 + linear lr at a quarter of the base rates.

Prints one JSON line; --out also writes it (profiles/schedule_run.json is a recorded run).
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "target-allocation-ppo-transformer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def step_child(a):
    """One process, one build: per minibatch size the median ms per step of each mode."""
    import torch
    from uavhip import _lib
    from uavhip.policy import TransformerActorCritic
    from uavhip.train import FusedPPOTrainer
    # two trainers alternate in every child, so that every build is timed under the same cache traffic:
    # a build without the entry point alternates two by-value trainers (the first is reported)
    modes = ("by_value", "hyper" if hasattr(_lib.LIB, "uavhip_ppo_step_hyper") else "by_value_twin")
    out = {}
    for mb in a.minibatches:
        n = a.graph_steps * mb
        g = torch.Generator().manual_seed(1)
        bufs = [torch.randn(n, 5, 14, generator=g) * 0.5, torch.randint(0, 2, (n,), generator=g),
                -0.69 + 0.05 * torch.randn(n, generator=g)] + [torch.randn(n, generator=g) for _ in range(3)]
        bufs = [t.cuda() for t in bufs]
        trainers = {}
        for mode in modes:
            torch.manual_seed(0)
            tr = FusedPPOTrainer(TransformerActorCritic().cuda(), mb)
            tr.set_buffers(*bufs)
            if mode == "hyper":
                tr.set_hyper()
            tr.perm[:n].copy_(torch.randperm(n, generator=torch.Generator().manual_seed(2)))
            trainers[mode] = (tr, tr.capture())
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = {mode: [] for mode in modes}
        for i in range(a.warmup + a.reps):
            for mode in modes:  # alternating, sample by sample
                ev[0].record()
                trainers[mode][1].replay()
                ev[1].record()
                ev[1].synchronize()
                if i >= a.warmup:
                    ms[mode].append(ev[0].elapsed_time(ev[1]) / a.graph_steps)
        out[str(mb)] = {mode: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
                        for mode, v in ms.items()}
        del trainers
        torch.cuda.empty_cache()
    print("CHILD " + json.dumps(out), flush=True)


def step_times(a):
    """--rounds rounds of one child per build -> per minibatch and variant the medians of the rounds."""
    def child(lib):
        env = dict(os.environ)
        env.pop("UAVHIP_LIB", None)
        if lib:
            env["UAVHIP_LIB"] = os.path.abspath(lib)
            env["UAVHIP_ACCEPT_PREV_ABI"] = "1"  # the parent build has no uavhip_ppo_step_hyper
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--minibatches", *map(str, a.minibatches),
               "--graph-steps", str(a.graph_steps), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            raise RuntimeError(f"step child failed ({lib or 'this build'}): {res.stderr[-2000:]}")
        return json.loads(next(x for x in res.stdout.splitlines() if x.startswith("CHILD "))[6:])

    rounds = {"parent": [], "by_value": [], "hyper": []}
    for _ in range(a.rounds):
        if a.parent_lib:
            rounds["parent"].append({mb: v["by_value"] for mb, v in child(a.parent_lib).items()})
        own = child(None)
        for mode in ("by_value", "hyper"):
            rounds[mode].append({mb: v[mode] for mb, v in own.items()})
    res = {"timing": f"HIP events around one replay of a {a.graph_steps}-step epoch graph / {a.graph_steps}; median of "
                     f"{a.reps} after {a.warmup}; {a.rounds} rounds, one process per build and round",
           "protocol": "every process alternates two trainers sample by sample: this build by_value / hyper; the "
                       "parent build two by-value trainers, the first reported (mode parent = uavhip_ppo_step of the "
                       "--parent-lib build through UAVHIP_LIB)",
           "trainers_per_process": 2, "parent_lib": bool(a.parent_lib)}
    for mb in map(str, a.minibatches):
        r = {}
        for name, rs in rounds.items():
            med = [x[mb]["median_ms"] for x in rs]
            if med:
                r[name] = {"median_of_medians_ms": statistics.median(med), "medians_ms": med,
                           "medians_min_max_ms": [min(med), max(med)],
                           "samples_min_max_ms": [min(x[mb]["min_ms"] for x in rs), max(x[mb]["max_ms"] for x in rs)]}
        res["minibatch_" + mb] = r
    return res


def eval_points(path):
    keys = ("iteration", "eval_mean_J", "eval_mean_J_baseline", "eval_beats_baseline", "entropy", "approx_kl",
            "clip_frac", "lr_actor", "entropy_coef")
    with open(path) as fh:
        return [{k: x.get(k) for k in keys} for x in map(json.loads, fh) if "eval_mean_J" in x]


def learn(a, tmp):
    import torch
    from uavhip.config import cfg
    from uavhip.fit import TrainingRun
    shape = dict(envs=a.envs, uavs=a.uavs, targets=a.targets, horizon=a.horizon, minibatch=a.minibatch, seed=a.seed,
                 eval_every=a.eval_every, eval_scenes=a.eval_scenes, eval_seed=a.eval_seed)
    K = a.iterations
    res = {"shape": shape, "iterations": K, "runs": {}}

    def run(name, iterations, **kw):
        t0 = time.perf_counter()
        r = TrainingRun(out_dir=os.path.join(tmp, name), **{**shape, **kw})
        r.fit(iterations)
        res["runs"][name] = {"arguments": {k: v for k, v in kw.items() if k != "init"}, "iterations": iterations,
                             "wall_s": time.perf_counter() - t0, "entropy_last": r.last["entropy"],
                             "eval": eval_points(os.path.join(tmp, name, "progress.jsonl"))}
        print(name, [(p["iteration"], round(p["eval_mean_J"], 3)) for p in res["runs"][name]["eval"]], file=sys.stderr,
              flush=True)
        del r
        torch.cuda.empty_cache()

    if K > 0:
        run("constant", K)
        run("linear_lr", K, lr_schedule="linear", lr_final_frac=0.1, schedule_iterations=K)
        run("linear_lr_entropy", K, lr_schedule="linear", lr_final_frac=0.1, entropy_schedule="linear",
            entropy_final_frac=0.0, schedule_iterations=K)
    if a.init_iterations > 0:
        from uavhip.imitate import ImitationRun
        J = a.init_iterations
        t0 = time.perf_counter()
        im = ImitationRun(a.envs, a.uavs, a.targets, a.minibatch, os.path.join(tmp, "dagger"), seed=a.seed,
                          assign_weight=16.0, source="dagger", expert_share=0.25, eval_every=a.init_eval_every,
                          eval_scenes=a.eval_scenes, eval_seed=a.eval_seed)
        final = im.fit(J)["final_model"]
        res["dagger"] = {"iterations": J, "wall_s": time.perf_counter() - t0,
                         "eval": eval_points(os.path.join(tmp, "dagger", "progress.jsonl"))}
        del im
        torch.cuda.empty_cache()
        run("init_constant", J, init=final, eval_every=a.init_eval_every)
        run("init_warmup_quarter_lr_linear", J, init=final, eval_every=a.init_eval_every, lr_actor=cfg.LR_ACTOR / 4, lr_critic=cfg.LR_CRITIC / 4,
            lr_warmup=5, lr_schedule="linear", lr_final_frac=0.1, schedule_iterations=J)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="(internal) time the steps of the loaded build")
    ap.add_argument("--parent-lib", default=None, help="libuavhip.so of the parent commit (omit: two variants)")
    ap.add_argument("--minibatches", type=int, nargs="+", default=[4096, 64])
    ap.add_argument("--graph-steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--minibatch", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=300, help="of each from-scratch run (0: skip)")
    ap.add_argument("--init-iterations", type=int, default=60, help="of the DAgger clone and the runs from it (0: skip)")
    ap.add_argument("--eval-every", type=int, default=25)
    ap.add_argument("--init-eval-every", type=int, default=10)
    ap.add_argument("--eval-scenes", type=int, default=1024)
    ap.add_argument("--eval-seed", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return step_child(a)
    res = {"step": step_times(a) if a.rounds > 0 else None}
    print("step", json.dumps(res["step"]), file=sys.stderr, flush=True)
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    tmp = tempfile.mkdtemp(prefix="schedule_bench_")
    try:
        res["learn"] = learn(a, tmp)
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
