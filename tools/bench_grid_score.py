"""Grid scores at BASELINE config C5 (100 000 sites x 100 times, C2 model), Q = 1 and Q = 5:
  * grid_scores (Predictor.score_grid + one host read) against what there was before it: predict_all_times, then numpy
    nanmean per site and per time and the per-mask metrics on the host -- alternating, medians, peak device memory of
    both (torch.cuda.max_memory_allocated);
  * stdadk_grid_score_f32 alone on a resident prediction buffer (device events): its algorithmic bytes
    rows (4Q + 5) + the accumulators over its time, beside the rate stdadk_rbf_build_f32 reaches on the same box
    (C2 features of 65 536 rows, past the Infinity Cache).
Every GPU step is a child process under its own time limit; the first one that fails ends the run.  One JSON line each.
usage (MI355X): python tools/bench_grid_score.py [--reps 5]
(kernel times: `rocprofv3 --kernel-trace --stats -- python tools/bench_grid_score.py --child 5`)"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--child", type=int, default=0, help="run one step in this process: the head width Q")
ap.add_argument("--sites", type=int, default=100000)
ap.add_argument("--times", type=int, default=100)
args = ap.parse_args()
if not args.child:
    for Q in (1, 5):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(Q), "--reps", str(args.reps),
                        "--sites", str(args.sites), "--times", str(args.times)], check=True, timeout=420)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
from stnf import _native as N
from stnf.models import STInterpMLP
from stnf.utils.predictions import grid_scores, predict_all_times

d = torch.device("cuda:0")
torch.manual_seed(0)
Q, S, T = args.child, args.sites, args.times
levels = [0.05, 0.25, 0.5, 0.75, 0.95][:Q] if Q > 1 else None
config = {"regression_type": "multi-quantile", "quantile_levels": levels, "interval": (levels[0], levels[-1])} if Q > 1 \
    else {"regression_type": "mean"}
m = STInterpMLP(p=0, k_spatial_centers=[1024, 4096, 5184], k_temporal_centers=[10, 15, 45], hidden_dims=[256, 256, 128],
                dropout=0.1, layernorm=True, output_dim=Q).to(d).eval()
rs = np.random.RandomState(0)
coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
z = rs.standard_normal((T, S)).astype(np.float32)
u = rs.uniform(size=z.shape)
z[u < 0.05] = np.nan
u = rs.uniform(size=z.shape)
masks = (u < 0.85, (u >= 0.85) & (u < 0.92), u >= 0.92)        # test: the 8 % that were not observed


def before():
    """predict_all_times -> host float64 grid -> nanmean per site / time -> per-mask metrics"""
    pred = predict_all_times(m, coords, T)
    err = pred - z
    out = {"site_mse": np.nanmean(err ** 2, axis=0), "time_mse": np.nanmean(err ** 2, axis=1)}
    for name, mask in zip(("train", "valid", "test"), masks):
        e = err[mask & np.isfinite(z)]
        out[name] = (float(np.mean(e ** 2)), float(np.mean(np.abs(e))))
    return out


def after():
    return grid_scores(m, z, coords, *masks, config=config)


a, b = before(), after()
assert np.allclose(a["site_mse"], b["site_mse"], rtol=1e-9) and np.allclose(a["time_mse"], b["time_mse"], rtol=1e-9)
for name in ("train", "valid", "test"):
    assert abs(a[name][0] - b["splits"][name]["mse"]) <= 1e-9 * a[name][0], name
ts, peak = {"before": [], "after": []}, {}
for _ in range(args.reps):
    for name, fn in (("before", before), ("after", after)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts[name].append((time.perf_counter() - t0) * 1e3)
        peak[name] = torch.cuda.max_memory_allocated() - base


def events(fn, reps):
    fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e-3


# the kernel alone on a resident buffer, and the HBM rate rbf_build reaches here
y = torch.randn(T * S, Q, device=d)
zt, ct = torch.from_numpy(z).to(d), torch.from_numpy((masks[0] * 1 + masks[1] * 2 + masks[2] * 3).astype(np.uint8)).to(d)
accs = (torch.zeros(4, N.GRID_SLOTS, dtype=torch.float64, device=d), torch.zeros(4, S, 3, dtype=torch.float64, device=d),
        torch.zeros(4, T, 3, dtype=torch.float64, device=d))
ws = torch.empty(N.grid_score_workspace_bytes(S, T) // 8, dtype=torch.float64, device=d)
lo, hi = (0, Q - 1) if Q > 1 else (-1, -1)
k_dt = events(lambda: [N.grid_score(y, zt, ct, Q // 2, levels, lo, hi, *accs, ws) for _ in range(10)], 10) / 10
k_bytes = S * T * (4 * Q + 5) + 2 * accs[1].numel() * 8 + accs[2].numel() * 8 + accs[0].numel() * 16
B = 65536
feats = torch.empty(B, (m.input_dim + 31) // 32 * 32, device=d)
c, t = torch.rand(B, 2, device=d), torch.rand(B, device=d)
r_dt = events(lambda: N.rbf_build(c, t, None, m.spatial_basis.centers, m.spatial_basis._bandwidths, "wendland",
                                  m.temporal_basis.centers, m.temporal_basis.bandwidths, feats), 20)
r_bytes = B * (12 + 4 * m.input_dim)
print(json.dumps({
    "Q": Q, "sites": S, "times": T, "reps": args.reps,
    "before_ms": statistics.median(ts["before"]), "after_ms": statistics.median(ts["after"]),
    "ratio_before_over_after": statistics.median(ts["before"]) / statistics.median(ts["after"]),
    "before_ms_all": [round(x, 1) for x in ts["before"]], "after_ms_all": [round(x, 1) for x in ts["after"]],
    "peak_device_bytes": peak,
    "kernel_ms": k_dt * 1e3, "kernel_bytes": k_bytes, "kernel_TBps": k_bytes / k_dt / 1e12,
    "rbf_build_TBps": r_bytes / r_dt / 1e12, "kernel_over_rbf_build": (k_bytes / k_dt) / (r_bytes / r_dt)}), flush=True)
