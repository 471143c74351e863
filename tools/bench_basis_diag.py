"""Basis diagnostics (stdadk_basis_diag_f32) at the two real shapes -- 10 000 sites x the C2 knot table (10 304 knots,
levels 1 024 / 4 096 / 5 184) and x the shipped 227 knots (25 / 81 / 121) -- with site weights and a site value: device
time per call (HIP events around batches of calls, median) and per kernel (the library's own event profiler), the
pairs per second that gives; the numpy float64 host path (stnf.utils.basis_diag.basis_diag_sums_host) on the same
shape with at most 16 threads, the only baseline there is; stdadk_group_norms_f32 on the C2 first layer in both
layouts; and what grid_scores costs with and without `basis_diagnostics` at the shape of profiles/grid_score.md
(--grid: 100 000 sites x 100 times, the C2 model).  Every GPU step is a child process under its own time limit; the
first one that fails ends the run.  One JSON line each.
usage (MI355X): python tools/bench_basis_diag.py [--reps 5] [--grid]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--child", default="", help="run one step in this process: c2 | default227 | grid")
ap.add_argument("--sites", type=int, default=10000)
ap.add_argument("--grid", action="store_true", help="also time grid_scores with and without the key")
ap.add_argument("--grid-sites", type=int, default=100000)
args = ap.parse_args()
if not args.child:
    for what in ("default227", "c2") + (("grid",) if args.grid else ()):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(args.reps),
                        "--sites", str(args.grid_sites if what == "grid" else args.sites)], check=True, timeout=420)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
torch.set_num_threads(min(16, torch.get_num_threads()))
from stnf import _native as N
from stnf.models import STInterpMLP
from stnf.utils import basis_diag as BD

LEVELS = {"c2": [1024, 4096, 5184], "default227": [25, 81, 121], "grid": [1024, 4096, 5184]}[args.child]
S = args.sites
d = torch.device("cuda:0")
rs = np.random.RandomState(0)
CALLS = 3


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS


if args.child == "grid":
    # grid_scores at the shape of profiles/grid_score.md: 100 000 sites x 100 times, the C2 model
    from stnf.utils import grid_scores
    T = 100
    torch.manual_seed(0)
    m = STInterpMLP(p=0, k_spatial_centers=LEVELS, k_temporal_centers=[10, 15, 45], hidden_dims=[256, 256, 128],
                    dropout=0.0).to(d).eval()
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = rs.standard_normal((T, S)).astype(np.float32)
    u = rs.uniform(size=z.shape)
    masks = [u < 0.85, (u >= 0.85) & (u < 0.92), u >= 0.92]
    out = {}
    for key in (False, True, False, True):
        grid_scores(m, z[:2], coords, *[k[:2] for k in masks], config={"basis_diagnostics": key})      # warm-up
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grid_scores(m, z, coords, *masks, config={"basis_diagnostics": key})
            ts.append(time.perf_counter() - t0)
        out.setdefault("with_key" if key else "without_key", []).append(statistics.median(ts))
    print(json.dumps({"grid_scores_seconds": out, "sites": S, "times": T, "knots": sum(LEVELS), "reps": args.reps}),
          flush=True)
    sys.exit(0)

torch.manual_seed(0)
sb = STInterpMLP(p=0, k_spatial_centers=LEVELS, k_temporal_centers=[10], hidden_dims=[16], dropout=0.0).spatial_basis
centers, bw = sb.centers.numpy().copy(), sb.bandwidths.numpy().copy()
Ks = len(centers)
coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
w = rs.randint(0, 100, S).astype(np.float64)
v = rs.uniform(0, 1, S)
ct, bt, xt = (torch.from_numpy(a).to(d) for a in (centers, bw, coords))
wt, vt = torch.from_numpy(w).to(d), torch.from_numpy(v).to(d)
knot = torch.zeros(Ks, 7, dtype=torch.float64, device=d)
site = torch.zeros(S, len(LEVELS), 3, dtype=torch.float64, device=d)
ws = torch.empty(N.basis_diag_workspace_bytes(S, Ks) // 8, dtype=torch.float64, device=d)
res = {"shape": args.child, "sites": S, "knots": Ks, "levels": LEVELS, "reps": args.reps, "pairs": S * Ks,
       "workspace_MiB": ws.numel() * 8 / 2 ** 20, "ms_per_call": {}, "kernel_ms": {}}
for basis in ("wendland", "gaussian", "triangular"):
    fn = lambda: N.basis_diag(ct, bt, basis, LEVELS, xt, wt, vt, BD.default_rho(basis), knot, site, ws)      # noqa: E731
    fn()                                                    # warm-up: code objects
    torch.cuda.synchronize()
    res["ms_per_call"][basis] = statistics.median(events(fn) for _ in range(args.reps))
    N.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    res["kernel_ms"][basis] = {name.split("<")[0]: ms for name, ms in N.profile_collect()}
    N.profile_enable(False)
res["in_support_wendland"] = None
fn = lambda: N.basis_diag(ct, bt, "wendland", LEVELS, xt, wt, vt, 1.0, knot, site, ws)      # noqa: E731
fn()
res["in_support_wendland"] = float(site[:, :, 0].sum().item())
res["pairs_per_s"] = {k: S * Ks / (ms * 1e-3) for k, ms in res["ms_per_call"].items()}

# the host path on the same shape (numpy float64, the threads this process was given, 16 at the most)
t0 = time.perf_counter()
hk, hs = BD.basis_diag_sums_host(centers, bw, "wendland", LEVELS, coords, w, v)
res["host_numpy_seconds"] = time.perf_counter() - t0
res["host_equals_device_counts"] = bool(np.array_equal(hk[:, 0], knot.cpu().numpy()[:, 0])
                                        and np.array_equal(hs[:, :, 0], site.cpu().numpy()[:, :, 0]))

# the group norms of a C2-sized first layer (256 x (Ks + 70)), both layouts
H, D = 256, Ks + 70
W0 = torch.randn(H, D, device=d)
W0t = W0.t().contiguous()
out = torch.empty(D, dtype=torch.float64, device=d)
res["group_norms_ms"] = {}
for name, (wgt, tr) in (("cols_of_W0", (W0, False)), ("rows_of_W0T", (W0t, True))):
    g = lambda: N.group_norms(wgt, tr, H, 0, D, out)      # noqa: E731
    g()
    torch.cuda.synchronize()
    res["group_norms_ms"][name] = statistics.median(events(g) for _ in range(args.reps))
print(json.dumps(res), flush=True)
