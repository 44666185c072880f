#!/usr/bin/env python3
"""What the constraints cost the exchange-move local search (uavhip_search_assignments_constrained,
DESIGN.md 9h), in one process on one GPU at 4096 scenes x 16 x 32, caps 32 / 32, from the empty start:

  search       k_search (uavhip_search_assignments), the yardstick: unchanged code, 0.42-0.44 ms in
               profiles/search_bench.json
  neutral      k_search_constrained with neutral arrays (all allowed, none fixed, capacity N): the same
               allocations bitwise, so the difference is what carrying the constraints costs
  constrained  k_search_constrained with a seeded mask of density 0.7, capacities uniform in {1, 2, 3}
               and each UAV committed with probability 0.2 to a uniform target or to none

by HIP events, the three launches ALTERNATING on the same scenes (scripts/search_bench.py's protocol):
median of --launches after --warmup. Also mean J, sweeps and exchanges of each. Timings are recorded, not
asserted. Prints one JSON line; --out also writes it (profiles/constrained_bench.json is a recorded run,
--session names it).
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
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--uavs", type=int, default=16)
    ap.add_argument("--targets", type=int, default=32)
    ap.add_argument("--sweeps", type=int, default=32)
    ap.add_argument("--exchanges", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--session", default=None, help="a name for the recorded run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from uavhip.vec_env import VecUAVEnv
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    S, N, M, R, X = a.scenes, a.uavs, a.targets, a.sweeps, a.exchanges
    env = VecUAVEnv(S, N, M, device=dev, seed=a.seed, full_reset_period=0, scene_buffers=1)
    env.generate_scenes()

    g = torch.Generator().manual_seed(a.seed)
    allowed = (torch.rand(S, N, M, generator=g) < 0.7).to(torch.uint8).to(dev)
    capacity = torch.randint(1, 4, (S, M), generator=g, dtype=torch.int32).to(dev)
    fixed_to = torch.randint(-1, M, (S, N), generator=g, dtype=torch.int32)
    committed = torch.rand(S, N, generator=g) < 0.2
    ids = env.tgt_id.cpu()  # the committed UAVs' targets as ids, list index -> tgt_id
    start = torch.where(committed & (fixed_to >= 0), torch.gather(ids, 1, fixed_to.clamp(min=0).long()),
                        torch.full((S, N), -1, dtype=torch.int32)).to(dev)
    fixed = committed.to(torch.uint8).to(dev)
    neutral = (torch.ones(S, N, M, dtype=torch.uint8, device=dev), torch.zeros(S, N, dtype=torch.uint8, device=dev),
               torch.full((S, M), N, dtype=torch.int32, device=dev))

    def bufs(n_stats):
        return dict(out=torch.empty(S, N, dtype=torch.int32, device=dev), J=torch.empty(S, dtype=torch.float64, device=dev),
                    covered=torch.empty(S, dtype=torch.int32, device=dev),
                    stats=torch.empty(S, n_stats, dtype=torch.int32, device=dev))

    b = {"search": bufs(6), "neutral": bufs(8), "constrained": bufs(8)}
    caps = dict(max_exchanges=X, max_sweeps=R)
    calls = {"search": lambda: env.search_assignments(None, **caps, **b["search"]),
             "neutral": lambda: env.search_assignments_constrained(None, *neutral, **caps, **b["neutral"]),
             "constrained": lambda: env.search_assignments_constrained(start, allowed, fixed, capacity, **caps,
                                                                       **b["constrained"])}
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
          for k in calls}
    for i in range(a.warmup + a.launches):
        j = i - a.warmup
        for k, fn in calls.items():
            if j >= 0:
                ev[k][j][0].record()
            fn()
            if j >= 0:
                ev[k][j][1].record()
    torch.cuda.synchronize()

    def stat(ms):
        ms = sorted(ms)
        return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}

    for k in ("out", "J", "covered"):
        assert torch.equal(b["search"][k], b["neutral"][k]), k
    assert torch.equal(b["search"]["stats"], b["neutral"]["stats"][:, :6])
    ms = {k: stat([s.elapsed_time(e) for s, e in v]) for k, v in ev.items()}

    def figures(k):
        st = b[k]["stats"].double()
        o = {"mean_J": float(b[k]["J"].mean()), "mean_covered": float(b[k]["covered"].double().mean()),
             "mean_sweeps": float(st[:, 0].mean()), "max_sweeps": int(st[:, 0].max()),
             "mean_exchanges": float(st[:, 4].mean()), "max_exchanges": int(st[:, 4].max()),
             "scan_not_clean": float((st[:, 5] == 0).double().mean())}
        if st.shape[1] == 8:
            o.update(mean_dropped=float(st[:, 6].mean()), mean_fixed_conflicts=float(st[:, 7].mean()))
        return o

    recorded = None
    path = os.path.join(ROOT, "profiles", "search_bench.json")
    if os.path.exists(path):
        with open(path) as f:
            recorded = json.load(f)["launch_ms_from_empty"]["search"]["median"]
    o = {"workload": f"{S} scenes x {N} x {M}, max_sweeps = {R}, max_exchanges = {X}, from the empty start",
         "constraints": "mask density 0.7, capacity uniform in {1, 2, 3}, each UAV committed with probability 0.2 to a "
                        "uniform target or to none",
         "session": a.session, "device": torch.cuda.get_device_name(0), "launches": a.launches, "warmup": a.warmup,
         "launch_ms": ms, "k_search_ms_in_profiles_search_bench_json": recorded,
         "neutral_over_search": ms["neutral"]["median"] / ms["search"]["median"],
         "constrained_over_search": ms["constrained"]["median"] / ms["search"]["median"],
         "search": figures("search"), "neutral": figures("neutral"), "constrained": figures("constrained")}
    print(json.dumps(o))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(o, indent=1) + "\n")


if __name__ == "__main__":
    main()
