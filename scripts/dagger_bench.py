#!/usr/bin/env python3
"""The expert-label kernel's cost and the first figures of imitation on the expert's labels
(uavhip.imitate --source expert / dagger), in one process on one GPU at 4096 x 16 x 32,
minibatch 4096. Everything is recorded, nothing asserted.

  kernel   k_expert_steps in follow mode (uavhip_expert_steps, actions_in = NULL, n_max = N * M, every
           output) beside k_teacher_steps given refine_assignments(None, max_sweeps=1): following the
           labels IS that allocation's walk, so both take the same steps. HIP events around each launch
           on a freshly reset env, the two alternating, median of --reps after --warmup launches of each.
  learn    --iterations ImitationRun iterations of each source (teacher, expert, dagger) with
           --assign-weight on the assign rows: eval_mean_J of the greedy decode every --eval-every
           iterations, label / assign agreement per iteration; then uavhip.fit --init from the dagger
           checkpoint; beside the baseline (the best-response search) and the one-sweep expert
           (refine_assignments(None, max_sweeps=1)) on the evaluation scenes.

Prints one JSON line; --out also writes it (profiles/dagger_run.json is a recorded run).
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


def kernel_times(E, N, M, seed, warmup, reps):
    import torch
    from uavhip import _lib
    from uavhip.vec_env import VecUAVEnv
    T = N * M
    dev = torch.device("cuda:0")
    env = VecUAVEnv(E, N, M, device=dev, seed=seed, full_reset_period=0, scene_buffers=1)
    env.generate_scenes()
    twin = VecUAVEnv(E, N, M, device=dev, seed=seed, full_reset_period=0, scene_buffers=1)
    twin.generate_scenes()
    asg = env.refine_assignments(None, max_sweeps=1)[0].clone()
    f64 = dict(dtype=torch.float64, device=dev)
    common = [dict(obs=torch.empty(T, E, 5, 14, device=dev), reward=torch.empty(T, E, **f64),
                   done=torch.empty(T, E, dtype=torch.uint8, device=dev)) for _ in range(2)]
    info = torch.empty(T, E, _lib.INFO_COUNT, **f64)
    labels = torch.empty(T, E, dtype=torch.int8, device=dev)
    margin = torch.empty(T, E, **f64)
    act = [torch.empty(T, E, dtype=torch.int8, device=dev) for _ in range(2)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_teacher, t_expert = [], []
    for i in range(warmup + reps):
        env.reset()
        twin.reset()
        ev[0].record()
        te = env.teacher_steps(asg, actions=act[0], info=info, **common[0])
        ev[1].record()
        ev[2].record()
        ex = twin.expert_steps(actions_out=act[1], labels=labels, margin=margin, **common[1])
        ev[3].record()
        torch.cuda.synchronize()
        if i >= warmup:
            t_teacher.append(ev[0].elapsed_time(ev[1]))
            t_expert.append(ev[2].elapsed_time(ev[3]))
    same = bool(torch.equal(act[0], act[1]) and torch.equal(common[0]["obs"], common[1]["obs"]) and
                torch.equal(common[0]["reward"], common[1]["reward"]) and torch.equal(te["steps"], ex["steps"]))
    rows = int((act[1] >= 0).sum())
    mt, mx = statistics.median(t_teacher), statistics.median(t_expert)
    return {"shape": [E, N, M], "n_max": T, "valid_rows": rows, "mean_episode_steps": float(ex["steps"].float().mean()),
            "label_1_share": float((labels == 1).sum()) / rows, "rejected_assigns": int(ex["stats"][:, 0].sum()),
            "reps": reps, "warmup": warmup, "timing": "HIP events around one launch, median",
            "k_teacher_steps_ms": mt, "k_teacher_steps_ms_min_max": [min(t_teacher), max(t_teacher)],
            "k_expert_steps_ms": mx, "k_expert_steps_ms_min_max": [min(t_expert), max(t_expert)],
            "ratio_expert_over_teacher": mx / mt, "valid_env_steps_per_s": rows / (mx * 1e-3),
            "same_walk_bitwise": same}


def eval_points(path):
    keys = ("iteration", "eval_mean_J", "eval_mean_J_baseline", "eval_beats_baseline")
    with open(path) as fh:
        return [{k: x.get(k) for k in keys} for x in map(json.loads, fh) if "eval_mean_J" in x]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--minibatch", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=60, help="of every clone and of the fit (0: kernel timing only)")
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--eval-scenes", type=int, default=1024)
    ap.add_argument("--eval-seed", type=int, default=1)
    ap.add_argument("--assign-weight", type=float, default=16.0)
    ap.add_argument("--expert-share", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from uavhip.fit import TrainingRun
    from uavhip.imitate import ImitationRun
    from uavhip.policy import TransformerActorCritic
    from uavhip.solve import AllocationSolver
    res = {"device": torch.cuda.get_device_name(0),
           "kernel": kernel_times(a.envs, a.uavs, a.targets, a.seed, a.warmup, a.reps)}
    print("kernel", res["kernel"]["ratio_expert_over_teacher"], file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    tmp = tempfile.mkdtemp(prefix="dagger_bench_")
    try:
        if a.iterations > 0:
            solver = AllocationSolver(TransformerActorCritic().to("cuda:0"), a.uavs, a.targets)
            res["eval_mean_J_baseline"] = float(solver.baseline(num_scenes=a.eval_scenes, seed=a.eval_seed).J.mean())
            res["eval_mean_J_one_sweep_expert"] = float(
                solver.baseline(num_scenes=a.eval_scenes, seed=a.eval_seed, max_sweeps=1).J.mean())
            del solver
            ev = dict(eval_every=a.eval_every, eval_scenes=a.eval_scenes, eval_seed=a.eval_seed)
            keys = ("iteration", "rows", "nll_before", "nll_after", "agreement", "assign_agreement", "fit_assign_agreement",
                    "label_agreement", "assign_share", "teacher_mean_J", "walked_mean_J", "rejected", "trace_ended")
            final = None
            for source in ("teacher", "expert", "dagger"):
                t0 = time.perf_counter()
                run = ImitationRun(a.envs, a.uavs, a.targets, a.minibatch, os.path.join(tmp, source), seed=a.seed,
                                   assign_weight=a.assign_weight, source=source, expert_share=a.expert_share, **ev)
                s = run.fit(a.iterations)
                with open(os.path.join(tmp, source, "progress.jsonl")) as fh:
                    lines = [json.loads(x) for x in fh]
                res[source] = {"iterations": a.iterations, "assign_weight": a.assign_weight,
                               "wall_s": time.perf_counter() - t0,
                               "curve": [{k: x.get(k) for k in keys} for x in lines],
                               "eval": eval_points(os.path.join(tmp, source, "progress.jsonl"))}
                print(source, res[source]["eval"], file=sys.stderr, flush=True)
                if source == "dagger":
                    res[source]["expert_share"] = a.expert_share
                    final = s["final_model"]
                del run
                torch.cuda.empty_cache()
            t0 = time.perf_counter()
            run = TrainingRun(out_dir=os.path.join(tmp, "fit"), init=final, envs=a.envs, uavs=a.uavs, targets=a.targets,
                              horizon=a.horizon, minibatch=a.minibatch, seed=a.seed, eval_every=a.eval_every,
                              eval_scenes=a.eval_scenes, eval_seed=a.eval_seed)
            run.fit(a.iterations)
            res["fit_from_dagger"] = {"iterations": a.iterations, "wall_s": time.perf_counter() - t0,
                                      "entropy_last": run.last["entropy"],
                                      "eval": eval_points(os.path.join(tmp, "fit", "progress.jsonl"))}
            print("fit", res["fit_from_dagger"]["eval"], file=sys.stderr, flush=True)
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
