"""Empirical variograms (stdadk_variogram_f32) at S' = 4 096 and 10 000 sites x 100 times, 1 and 4 lags, 15 bins: device
time per call (HIP events around batches of calls, median), the pair-slices per second that gives, with and without a
prediction; and, for scale only, the numpy float64 host path (stnf.utils.variogram.variogram_sums_host) at 1 000 sites
x 20 times.  Every GPU step is a child process under its own time limit; the first one that fails ends the run.  One
JSON line each.
usage (MI355X): python tools/bench_variogram.py [--reps 5]
(kernel times: `rocprofv3 --kernel-trace --stats -- python tools/bench_variogram.py --child 4096,4`)"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--child", default="", help="run one step in this process: SITES,LAGS")
ap.add_argument("--times", type=int, default=100)
ap.add_argument("--bins", type=int, default=15)
args = ap.parse_args()
if not args.child:
    for S in (4096, 10000):
        for L in (1, 4):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{S},{L}", "--reps", str(args.reps),
                            "--times", str(args.times), "--bins", str(args.bins)], check=True, timeout=300)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
from stnf import _native as N
from stnf.utils import variogram as V

S, L = (int(v) for v in args.child.split(","))
T, B = args.times, args.bins
d = torch.device("cuda:0")
rs = np.random.RandomState(0)
coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
z = rs.standard_normal((T, S)).astype(np.float32)
z[rs.uniform(size=z.shape) < 0.05] = np.nan
u = rs.uniform(size=z.shape)
code = (1 * (u < 0.85) + 2 * ((u >= 0.85) & (u < 0.92)) + 3 * (u >= 0.92)).astype(np.uint8)
edges = V.variogram_edges(coords, B)
e2 = edges * edges
y = torch.randn(T * S, 3, device=d)
zt, ct, xt = torch.from_numpy(z).to(d), torch.from_numpy(code).to(d), torch.from_numpy(coords).to(d)
acc = torch.zeros(4, L, B, 4, dtype=torch.float64, device=d)
ws = torch.empty(N.variogram_workspace_bytes(S, T, B, L) // 8, dtype=torch.float64, device=d)
CALLS = 3


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS


runs = {"with_prediction": lambda: N.variogram(y, 1, zt, ct, xt, e2, L, acc, ws),
        "field_only": lambda: N.variogram(None, 0, zt, ct, xt, e2, L, acc, ws)}
ms = {}
for k, fn in runs.items():
    fn()                                                    # warm-up: code objects
    torch.cuda.synchronize()
    ms[k] = statistics.median(events(fn) for _ in range(args.reps))
pair_slices = S * (S - 1) // 2 * T + sum(S * S * (T - lag) for lag in range(1, min(L, T)))
binned = float(acc[..., 0].sum().item())

# the host path, for scale: 1 000 sites x 20 times, the same lags
hs, ht = 1000, 20
t0 = time.perf_counter()
V.variogram_sums_host(rs.standard_normal((ht, hs)).astype(np.float32), z[:ht, :hs], code[:ht, :hs], coords[:hs], e2, L)
host_s = time.perf_counter() - t0
host_pairs = hs * (hs - 1) // 2 * ht + sum(hs * hs * (ht - lag) for lag in range(1, min(L, ht)))
print(json.dumps({"sites": S, "times": T, "lags": L, "bins": B, "reps": args.reps, "ms_per_call": ms,
                  "pair_slices": pair_slices, "pair_slices_counted_in_a_bin": binned,
                  "pair_slices_per_s": {k: pair_slices / (v * 1e-3) for k, v in ms.items()},
                  "workspace_MiB": ws.numel() * 8 / 2 ** 20,
                  "host_numpy": {"sites": hs, "times": ht, "seconds": host_s, "pair_slices_per_s": host_pairs / host_s}}),
      flush=True)
