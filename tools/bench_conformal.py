"""Conformal calibration: (1) stdadk_select_f32 alone at n in {1e5, 1e6, 1e7} x C in {1, 5} columns, one selection per
column at the level 0.9, against torch.kthvalue and torch.sort on the same tensor in the same process, alternating,
warm -- device time per call (HIP events around batches of calls, median over repetitions), the library's own event
profiler for the kernels of one call, and that the three agree on the values; (2) what `conformal: true` costs inside
grid_scores at the shape of profiles/grid_score.md (--grid: 100 000 sites x 100 times, the C2 model with five
quantiles), with and without the key, alternating, host clock around calls that end in the host read.  Every GPU step
is a child process under its own time limit; the first one that fails ends the run.  One JSON line each.
usage (MI355X): python tools/bench_conformal.py [--reps 5] [--grid]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--child", default="", help="run one step in this process: select | grid")
ap.add_argument("--grid", action="store_true", help="also time grid_scores with and without the key")
ap.add_argument("--grid-sites", type=int, default=100000)
args = ap.parse_args()
if not args.child:
    for what in ("select",) + (("grid",) if args.grid else ()):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(args.reps),
                        "--grid-sites", str(args.grid_sites)], check=True, timeout=420)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
torch.set_num_threads(min(16, torch.get_num_threads()))
from stnf import _native as N
from stnf import calibration as CF
from stnf.models import STInterpMLP

d = torch.device("cuda:0")
rs = np.random.RandomState(0)


def events(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


if args.child == "grid":
    from stnf.utils import grid_scores
    S, T = args.grid_sites, 100
    levels = [0.05, 0.25, 0.5, 0.75, 0.95]
    torch.manual_seed(0)
    m = STInterpMLP(p=0, k_spatial_centers=[1024, 4096, 5184], k_temporal_centers=[10, 15, 45],
                    hidden_dims=[256, 256, 128], dropout=0.0, output_dim=5).to(d).eval()
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = rs.standard_normal((T, S)).astype(np.float32)
    u = rs.uniform(size=z.shape)
    masks = [u < 0.85, (u >= 0.85) & (u < 0.92), u >= 0.92]
    base = {"regression_type": "multi-quantile", "quantile_levels": levels, "interval": (0.05, 0.95)}
    out, last = {}, None
    for key in (False, True, False, True):
        grid_scores(m, z[:2], coords, *[k[:2] for k in masks], config=dict(base, conformal=key))      # warm-up
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = grid_scores(m, z, coords, *masks, config=dict(base, conformal=key))
            ts.append(time.perf_counter() - t0)
        out.setdefault("with_key" if key else "without_key", []).append(statistics.median(ts))
    cf = last["conformal"]
    print(json.dumps({"grid_scores_seconds": out, "sites": S, "times": T, "Q": 5, "reps": args.reps,
                      "n_cal": cf["n_cal"], "n_eval": cf["n_eval"], "offset": cf["intervals"][0]["offset"],
                      "coverage_before": cf["intervals"][0]["coverage_before"],
                      "coverage_after": cf["intervals"][0]["coverage_after"]}), flush=True)
    sys.exit(0)

for n in (100000, 1000000, 10000000):
    for C in (1, 5):
        keys = torch.from_numpy(rs.standard_normal((C, n)).astype(np.float32)).to(d)
        nd = torch.tensor([n], dtype=torch.int64, device=d)
        sels = [(c, None, 0.9) for c in range(C)]
        k = CF.conformal_rank(n, 0.9) + 1
        value = torch.empty(C, dtype=torch.float32, device=d)
        used = torch.empty(C, dtype=torch.int64, device=d)
        ws = torch.empty(N.select_workspace_bytes(C) // 8, dtype=torch.float64, device=d)
        fns = {"select": lambda: N.select(keys, nd, sels, value, used, ws),
               "kthvalue": lambda: torch.kthvalue(keys, k, dim=1),
               "sort": lambda: torch.sort(keys, dim=1)}
        for fn in fns.values():                                 # warm-up: code objects, the allocator's blocks
            fn()
        torch.cuda.synchronize()
        calls = max(10, min(200, 200000000 // (n * C)))
        ms = {name: [] for name in fns}
        for _ in range(args.reps):
            for name, fn in fns.items():                        # alternating
                ms[name].append(events(fn, calls))
        fns["select"]()
        same = bool(torch.equal(value, torch.kthvalue(keys, k, dim=1).values)
                    and torch.equal(value, torch.sort(keys, dim=1).values[:, k - 1]))
        N.profile_enable(True)
        fns["select"]()
        torch.cuda.synchronize()
        kern = {}
        for name, t in N.profile_collect():
            kern[name] = kern.get(name, 0.0) + t
        N.profile_enable(False)
        print(json.dumps({"n": n, "C": C, "rank": k - 1, "calls_per_window": calls, "reps": args.reps,
                          "ms_per_call": {name: statistics.median(v) for name, v in ms.items()},
                          "ms_min_max": {name: [min(v), max(v)] for name, v in ms.items()},
                          "select_kernel_ms": kern, "values_equal": same,
                          "GB_per_s_of_one_read": {name: n * C * 4 / (statistics.median(v) * 1e-3) / 1e9
                                                   for name, v in ms.items()}}), flush=True)
