"""Quantile diagnostics at BASELINE config C5 (100 000 sites x 100 times, C2 model), Q = 1, 5, 8:
  * stdadk_quantile_diag_f32 beside stdadk_grid_score_f32 on the same resident prediction buffer (device events,
    alternating): time and achieved bytes/s over the bytes both read, rows (4Q + 5), plus each one's accumulators
    (grid_score.hip's kernels are the parent commit's: this change moved three helpers of theirs into a header);
  * grid_scores end to end with and without `quantile_diagnostics`, alternating, medians -- the run without the key is
    the default score_grid path, whose calls this change does not alter.
Every GPU step is a child process under its own time limit; the first one that fails ends the run.  One JSON line each.
usage (MI355X): python tools/bench_quantile_diag.py [--reps 5]
(kernel times: `rocprofv3 --kernel-trace --stats -- python tools/bench_quantile_diag.py --child 5`)"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--child", type=int, default=0, help="run one step in this process: the head width Q")
ap.add_argument("--sites", type=int, default=100000)
ap.add_argument("--times", type=int, default=100)
args = ap.parse_args()
if not args.child:
    for Q in (1, 5, 8):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(Q), "--reps", str(args.reps),
                        "--sites", str(args.sites), "--times", str(args.times)], check=True, timeout=300)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
from stnf import _native as N
from stnf.models import STInterpMLP
from stnf.utils.predictions import grid_scores

d = torch.device("cuda:0")
torch.manual_seed(0)
Q, S, T = args.child, args.sites, args.times
levels = [0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.95] if Q == 8 else [0.05, 0.25, 0.5, 0.75, 0.95][:Q] if Q > 1 else [0.5]
config = {"regression_type": "multi-quantile", "quantile_levels": levels, "interval": (levels[0], levels[-1])} if Q > 1 \
    else {"regression_type": "quantile", "current_quantile": 0.5}
m = STInterpMLP(p=0, k_spatial_centers=[1024, 4096, 5184], k_temporal_centers=[10, 15, 45], hidden_dims=[256, 256, 128],
                dropout=0.1, layernorm=True, output_dim=Q).to(d).eval()
rs = np.random.RandomState(0)
coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
z = rs.standard_normal((T, S)).astype(np.float32)
u = rs.uniform(size=z.shape)
z[u < 0.05] = np.nan
u = rs.uniform(size=z.shape)
masks = (u < 0.85, (u >= 0.85) & (u < 0.92), u >= 0.92)


def events(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e-3 for e0, e1 in ev]


# ---- the two reductions alone on one resident buffer, alternating
y = torch.randn(T * S, Q, device=d)
zt, ct = torch.from_numpy(z).to(d), torch.from_numpy((masks[0] * 1 + masks[1] * 2 + masks[2] * 3).astype(np.uint8)).to(d)
lo, hi = (0, Q - 1) if Q > 1 else (-1, -1)
g_accs = (torch.zeros(4, N.GRID_SLOTS, dtype=torch.float64, device=d), torch.zeros(4, S, 3, dtype=torch.float64, device=d),
          torch.zeros(4, T, 3, dtype=torch.float64, device=d))
q_accs = (torch.zeros(4, N.QD_SLOTS, dtype=torch.float64, device=d), torch.zeros(4, S, 4, dtype=torch.float64, device=d),
          torch.zeros(4, T, 4, dtype=torch.float64, device=d))
g_ws = torch.empty(N.grid_score_workspace_bytes(S, T) // 8, dtype=torch.float64, device=d)
q_ws = torch.empty(N.quantile_diag_workspace_bytes(S, T) // 8, dtype=torch.float64, device=d)
CALLS = 10
runs = {"grid_score": lambda: [N.grid_score(y, zt, ct, Q // 2, levels, lo, hi, *g_accs, g_ws) for _ in range(CALLS)],
        "quantile_diag": lambda: [N.quantile_diag(y, zt, ct, levels, lo, hi, *q_accs, q_ws) for _ in range(CALLS)]}
for fn in runs.values():
    fn()                                                    # warm-up: code objects
kt = {k: [] for k in runs}
for _ in range(args.reps):
    for k, fn in runs.items():
        kt[k] += events(fn, 2)
rows_bytes = S * T * (4 * Q + 5)
k_bytes = {"grid_score": rows_bytes + 2 * g_accs[1].numel() * 8 + g_accs[2].numel() * 8,
           "quantile_diag": rows_bytes + 2 * q_accs[1].numel() * 8 + q_accs[2].numel() * 8}
k_ms = {k: statistics.median(v) / CALLS * 1e3 for k, v in kt.items()}

# ---- grid_scores end to end, with and without the key
variants = {"plain": config, "diagnostics": dict(config, quantile_diagnostics=True)}
out = {k: grid_scores(m, z, coords, *masks, config=c) for k, c in variants.items()}           # warm-up, and the check
assert "quantile" in out["diagnostics"] and "quantile" not in out["plain"]
np.testing.assert_equal(out["plain"]["splits"], out["diagnostics"]["splits"])      # (an empty split's metrics are NaN)
qd = out["diagnostics"]["quantile"]["all"]
crps = out["plain"]["splits"]["all"].get("crps", 2.0 * out["plain"]["splits"]["all"].get("check_loss", float("nan")))
assert abs(qd["crps"] - crps) <= 1e-9 * abs(crps), (qd["crps"], crps)
ts = {k: [] for k in variants}
for _ in range(args.reps):
    for k, c in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid_scores(m, z, coords, *masks, config=c)
        torch.cuda.synchronize()
        ts[k].append((time.perf_counter() - t0) * 1e3)
print(json.dumps({
    "Q": Q, "sites": S, "times": T, "reps": args.reps,
    "kernel_ms": k_ms, "kernel_ms_all": {k: [round(x / CALLS * 1e3, 4) for x in v] for k, v in kt.items()},
    "kernel_bytes": k_bytes, "kernel_TBps": {k: k_bytes[k] / (k_ms[k] * 1e-3) / 1e12 for k in k_ms},
    "quantile_diag_over_grid_score_time": k_ms["quantile_diag"] / k_ms["grid_score"],
    "grid_scores_ms": {k: statistics.median(v) for k, v in ts.items()},
    "grid_scores_ms_all": {k: [round(x, 1) for x in v] for k, v in ts.items()},
    "cross_rate_all": qd["cross_rate"], "crps_all": qd["crps"]}), flush=True)
