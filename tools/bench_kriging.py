"""Local ordinary kriging (stdadk_krige_weights_f64, stdadk_krige_apply_f32, grid_baselines with `baseline_kriging`) at
its real shapes:
  weights  the weights call on the table of 10 000 and 100 000 sites (40 % of them sources, leave-one-out), k = 8 and
           16, shared (one slice) and 100 slices (the per-time route's rows: the shared table repeated, the solves do
           not depend on the data for their time).  Beside it, on the same systems: torch.linalg.solve, batched, on
           the device (up to 10^6 rows: its matrices are 2 KiB a row at k = 16), and kriging_weights_host (numpy float64)
           on the host of the same box for the 10 000-row shapes.  Useful operations per row, counted here: the
           factorisation k^3 / 3, two right sides forward and back 4 k^2, the k^2 correlations not counted.
  apply    the apply call, 100 slices, Q = 1 and Q = 4: bytes moved over time.
  grid     grid_baselines at --grid-sites x 100 times on site-wise masks (one shared table) without the key and with
           `baseline_kriging` (exponential, given parameters; and fitted), alternating; and on per-entry masks for
           --pertime-slices slices (a search and a solve per slice) with and without the key.
Device time is HIP events around batches of calls, median; per kernel the library's own event profiler.  Every GPU step
is a child process under its own time limit; the first one that fails ends the run.  One JSON line each.
usage (MI355X): python tools/bench_kriging.py [--reps 5] [--grid]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--child", default="", help="run one step in this process: weights | apply | grid")
ap.add_argument("--grid", action="store_true", help="also time grid_baselines with and without the key")
ap.add_argument("--grid-sites", type=int, default=100000)
ap.add_argument("--pertime-slices", type=int, default=10)
args = ap.parse_args()
if not args.child:
    for what in ("weights", "apply") + (("grid",) if args.grid else ()):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(args.reps), "--grid-sites",
               str(args.grid_sites), "--pertime-slices", str(args.pertime_slices)]
        subprocess.run(cmd, check=True, timeout=420)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
torch.set_num_threads(min(16, torch.get_num_threads()))
from stnf import _native as N
from stnf.utils import baselines as BL
from stnf.utils import kriging as KR

d = torch.device("cuda:0")
rs = np.random.RandomState(0)
CALLS = 3
F64_VECTOR_PEAK = 78.6e12                       # FLOP/s, the MI355X's public float64 vector specification
PARAMS = (0.1, 1.0, 0.05)                       # nugget, psill, range: a few neighbours inside the range


def events(fn, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def table(S, k):
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    src = np.zeros((1, S), dtype=np.uint8)
    src[0, rs.choice(S, int(0.4 * S), replace=False)] = 1
    ct = torch.from_numpy(coords).to(d)
    idx, d2 = BL.device_knn(ct, ct, torch.from_numpy(src).to(d), k, True)
    return coords, ct, idx, d2


if args.child == "weights":
    for S in (10000, 100000):
        for k in (8, 16):
            coords, ct, idx1, d21 = table(S, k)
            for slices in (1, 100):
                idx, d2 = idx1.expand(slices, S, k).contiguous(), d21.expand(slices, S, k).contiguous()
                rows = slices * S
                w = torch.empty((slices, S, k), dtype=torch.float64, device=d)
                var = torch.empty((slices, S), dtype=torch.float64, device=d)
                res = {"step": "weights", "sites": S, "slices": slices, "rows": rows, "k": k}
                for model in (0, 1):
                    fn = lambda: N.krige_weights(idx, d2, k, ct, model, *PARAMS, w, var)      # noqa: E731
                    fn()
                    torch.cuda.synchronize()
                    ms = statistics.median(events(fn) for _ in range(args.reps))
                    flops = rows * (k ** 3 / 3.0 + 4.0 * k * k)
                    res[KR.MODELS[model]] = {"ms_per_call": ms, "rows_per_s": rows / (ms * 1e-3),
                                             "useful_gflops": flops / (ms * 1e-3) / 1e9,
                                             "fraction_of_f64_vector_peak": flops / (ms * 1e-3) / F64_VECTOR_PEAK,
                                             "bytes_GB_per_s": rows * k * (4 + 8 + 8 + 8) / (ms * 1e-3) / 1e9}
                res["singular_rows"] = int(torch.isnan(var).sum())
                if rows <= 10 ** 6:              # the same systems through torch.linalg.solve, batched, on the device
                    xy = ct.double()[idx.reshape(rows, k).long()]
                    dist = torch.cdist(xy, xy)
                    K = PARAMS[1] * torch.exp(-dist / PARAMS[2]) + PARAMS[0] * torch.eye(k, dtype=torch.float64, device=d)
                    rhs = torch.stack([torch.ones((rows, k), dtype=torch.float64, device=d),
                                       PARAMS[1] * torch.exp(-d2.reshape(rows, k).sqrt() / PARAMS[2])], dim=2)
                    del xy, dist
                    solve = lambda: torch.linalg.solve(K, rhs)      # noqa: E731
                    solve()
                    torch.cuda.synchronize()
                    res["torch_linalg_solve_ms"] = statistics.median(events(solve, 1) for _ in range(args.reps))
                    del K, rhs
                if rows == 10000:
                    ih, dh = idx.cpu().numpy(), d2.cpu().numpy()
                    t0 = time.perf_counter()
                    hw, hv = KR.kriging_weights_host(ih, dh, k, coords, 1, *PARAMS)
                    res["kriging_weights_host_seconds"] = time.perf_counter() - t0
                    N.krige_weights(idx, d2, k, ct, 1, *PARAMS, w, var)
                    res["host_equals_device_spherical"] = bool(np.array_equal(hw, w.cpu().numpy(), equal_nan=True)
                                                               and np.array_equal(hv, var.cpu().numpy(), equal_nan=True))
                if slices == 100 and k == 16:
                    N.profile_enable(True)
                    N.krige_weights(idx, d2, k, ct, 0, *PARAMS, w, var)
                    torch.cuda.synchronize()
                    res["kernel_ms"] = {name.split("<")[0]: ms for name, ms in N.profile_collect()}
                    N.profile_enable(False)
                print(json.dumps(res), flush=True)
                del idx, d2, w, var
    sys.exit(0)

if args.child == "apply":
    for S in (10000, 100000):
        k, nT = 8, 100
        coords, ct, idx, d2 = table(S, k)
        w, var = KR.device_kriging_weights(idx, d2, k, ct, 0, *PARAMS)
        z = torch.from_numpy(rs.standard_normal((nT, S)).astype(np.float32)).to(d)
        for zq in ([0.0], [-1.2816, 0.0, 0.6745, 1.6449]):
            out = torch.empty((nT * S, len(zq)), dtype=torch.float32, device=d)
            fn = lambda: N.krige_apply(idx, w, var, k, z, zq, out)      # noqa: E731
            fn()
            torch.cuda.synchronize()
            ms = statistics.median(events(fn) for _ in range(args.reps))
            moved = nT * S * (k * 4 + 4 * len(zq)) + S * k * (4 + 8) + S * 8      # gathers of z and the output; the table once
            print(json.dumps({"step": "apply", "sites": S, "slices": nT, "k": k, "Q": len(zq), "ms_per_call": ms,
                              "entries_per_s": nT * S / (ms * 1e-3), "bytes_GB_per_s": moved / (ms * 1e-3) / 1e9}), flush=True)
    sys.exit(0)

S, T = args.grid_sites, 100
coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
z = (np.sin(6 * coords[:, 0]) * np.cos(4 * coords[:, 1]))[None, :] + 0.3 * rs.standard_normal((T, S))
z = z.astype(np.float32)
u = np.broadcast_to(rs.uniform(size=S), (T, S))                  # site-wise splits: one shared table
masks = [u < 0.85, (u >= 0.85) & (u < 0.92), u >= 0.92]
given = {"baseline_kriging": True, "kriging_params": (0.09, 0.15, 0.3), "kriging_levels": [0.05, 0.95]}
fitted = {"baseline_kriging": True, "kriging_levels": [0.05, 0.95]}
out = {}
BL.grid_baselines(z[:2], coords, *[m[:2] for m in masks], config=given, device=d)      # warm-up
for name, config in (("without_key", {}), ("with_key_given", given), ("with_key_fitted", fitted)) * 2:
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = BL.grid_baselines(z, coords, *masks, config=config, device=d)
        ts.append(time.perf_counter() - t0)
    out.setdefault(name, []).append(statistics.median(ts))
res = {"step": "grid", "grid_baselines_seconds": out, "sites": S, "times": T, "reps": args.reps, "masks": "site-wise",
       "kriging": {s: {n: got["kriging"]["splits"][s][n] for n in ("mse", "crps", "coverage")} for s in ("valid", "test")},
       "idw_mse": {s: got["idw"]["splits"][s]["mse"] for s in ("valid", "test")}, "msse": got["kriging"]["msse"],
       "variogram_fit": got["kriging"]["variogram_fit"], "n_singular": got["kriging"]["n_singular"]}
n = args.pertime_slices
v = rs.uniform(size=(n, S))
per = [v < 0.85, (v >= 0.85) & (v < 0.92), v >= 0.92]
BL.grid_baselines(z[:1], coords, *[m[:1] for m in per], config=given, device=d)
res["per_time"] = {"slices": n}
for name, config in (("without_key", {}), ("with_key_given", given)):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = BL.grid_baselines(z[:n], coords, *per, config=config, device=d)
    res["per_time"][name] = time.perf_counter() - t0
    assert not got["shared_table"]
print(json.dumps(res), flush=True)
