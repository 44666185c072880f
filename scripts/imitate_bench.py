#!/usr/bin/env python3
"""The teacher-forced episode kernel's cost and the first figures of the imitation warm start
(uavhip.imitate), in one process on one GPU at 4096 x 16 x 32, minibatch 4096. Everything
is recorded, nothing asserted.

  kernel   k_teacher_steps (uavhip_teacher_steps, n_max = N * M, every output) on the baseline teacher,
           beside uavhip_env_step replaying the SAME recorded action trace in one T = N * M launch
           (auto_reset = 0, every output): HIP events around each launch on a freshly reset env, the two
           alternating, median of --reps after --warmup launches of each. The replay is the yardstick:
           it does less (no action derivation, no steps / finished / ep_return / stats). At this shape
           it packs two envs into a wave; the same replay held to one env per wave is timed beside it.
  clone    --iterations ImitationRun iterations: NLL and agreement per iteration, eval_mean_J of the
           greedy decode every --eval-every iterations; and the same with --assign-weight on the assign rows
  fit      uavhip.fit for --iterations iterations from scratch and from the clone (--init), the same
           eval scenes and cadence, beside the non-learned baseline

Prints one JSON line; --out also writes it (profiles/imitate_run.json is a recorded run).
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
    asg = env.refine_assignments(None)[0].clone()
    f64 = dict(dtype=torch.float64, device=dev)
    bufs = [dict(obs=torch.empty(T, E, 5, 14, device=dev), reward=torch.empty(T, E, **f64),
                 done=torch.empty(T, E, dtype=torch.uint8, device=dev),
                 info=torch.empty(T, E, _lib.INFO_COUNT, **f64)) for _ in range(2)]
    actions = torch.empty(T, E, dtype=torch.int8, device=dev)
    env.reset()
    first = env.teacher_steps(asg, actions=actions, **bufs[0])
    trace = actions.clamp(min=0).contiguous()
    rows, steps = int((actions >= 0).sum()), first["steps"].clone()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    t_teacher, t_replay, t_single = [], [], []
    for i in range(warmup + reps):
        env.reset()
        twin.reset()
        ev[0].record()
        env.teacher_steps(asg, actions=actions, **bufs[0])
        ev[1].record()
        ev[2].record()
        twin.step(trace, auto_reset=False, obs_out=bufs[1]["obs"], reward_out=bufs[1]["reward"],
                  done_out=bufs[1]["done"], info_out=bufs[1]["info"])
        ev[3].record()
        # the same replay held to one env per wave (k_env_step: k_teacher_steps' mapping, plus the LDS
        # pair table); twin's outputs and end state are bitwise the same either way
        twin.reset()
        twin.desc.flags |= _lib.ENV_ONE_PER_WAVE
        ev[4].record()
        twin.step(trace, auto_reset=False, obs_out=bufs[1]["obs"], reward_out=bufs[1]["reward"],
                  done_out=bufs[1]["done"], info_out=bufs[1]["info"])
        ev[5].record()
        twin.desc.flags &= ~_lib.ENV_ONE_PER_WAVE
        torch.cuda.synchronize()
        if i >= warmup:
            t_teacher.append(ev[0].elapsed_time(ev[1]))
            t_replay.append(ev[2].elapsed_time(ev[3]))
            t_single.append(ev[4].elapsed_time(ev[5]))
    valid = actions >= 0
    same = bool(torch.equal(bufs[0]["reward"][valid], bufs[1]["reward"][valid]) and
                torch.equal(bufs[0]["obs"][1:][valid[:-1]], bufs[1]["obs"][:-1][valid[:-1]]))
    mt, mr, ms = statistics.median(t_teacher), statistics.median(t_replay), statistics.median(t_single)
    return {"shape": [E, N, M], "n_max": T, "valid_rows": rows, "mean_episode_steps": float(steps.float().mean()),
            "reps": reps, "warmup": warmup, "timing": "HIP events around one launch, median",
            "k_teacher_steps_ms": mt, "k_teacher_steps_ms_min_max": [min(t_teacher), max(t_teacher)],
            "env_step_replay_ms": mr, "env_step_replay_ms_min_max": [min(t_replay), max(t_replay)],
            "ratio_teacher_over_replay": mt / mr, "env_step_replay_one_env_per_wave_ms": ms,
            "env_step_replay_one_env_per_wave_ms_min_max": [min(t_single), max(t_single)],
            "ratio_teacher_over_one_env_per_wave_replay": mt / ms, "valid_env_steps_per_s": rows / (mt * 1e-3),
            "replay_rows_equal_bitwise": same}


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
    ap.add_argument("--iterations", type=int, default=60, help="of the clone and of both fits (0: kernel timing only)")
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--eval-scenes", type=int, default=1024)
    ap.add_argument("--assign-weight", type=float, default=16.0,
                    help="a second clone with this advantage on the assign rows (0: skip it)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from uavhip.fit import TrainingRun
    from uavhip.imitate import ImitationRun
    res = {"device": torch.cuda.get_device_name(0),
           "kernel": kernel_times(a.envs, a.uavs, a.targets, a.seed, a.warmup, a.reps)}
    torch.cuda.empty_cache()
    tmp = tempfile.mkdtemp(prefix="imitate_bench_")
    try:
        if a.iterations > 0:
            ev = dict(eval_every=a.eval_every, eval_scenes=a.eval_scenes)
            keys = ("iteration", "rows", "nll_before", "nll_after", "agreement_before", "agreement", "assign_agreement",
                    "assign_share", "teacher_mean_J", "walked_mean_J", "rejected")
            variants = [("clone", 1.0)] + ([("clone_assign_weighted", a.assign_weight)] if a.assign_weight > 0 else [])
            for name, weight in variants:
                t0 = time.perf_counter()
                clone = ImitationRun(a.envs, a.uavs, a.targets, a.minibatch, os.path.join(tmp, name), seed=a.seed,
                                     assign_weight=weight, **ev)
                s = clone.fit(a.iterations)
                with open(os.path.join(tmp, name, "progress.jsonl")) as fh:
                    lines = [json.loads(x) for x in fh]
                res[name] = {"iterations": a.iterations, "assign_weight": weight, "wall_s": time.perf_counter() - t0,
                             "curve": [{k: x.get(k) for k in keys} for x in lines],
                             "eval": eval_points(os.path.join(tmp, name, "progress.jsonl"))}
                if name == "clone":
                    summary = s
                del clone
                torch.cuda.empty_cache()
            shape = dict(envs=a.envs, uavs=a.uavs, targets=a.targets, horizon=a.horizon, minibatch=a.minibatch,
                         seed=a.seed)
            for name, init in (("fit_from_scratch", None), ("fit_from_clone", summary["final_model"])):
                t0 = time.perf_counter()
                run = TrainingRun(out_dir=os.path.join(tmp, name), init=init, **shape, **ev)
                run.fit(a.iterations)
                res[name] = {"iterations": a.iterations, "wall_s": time.perf_counter() - t0,
                             "entropy_last": run.last["entropy"], "mean_ep_reward_last": run.last["mean_ep_reward"],
                             "eval": eval_points(os.path.join(tmp, name, "progress.jsonl"))}
                del run
                torch.cuda.empty_cache()
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
