"""Neighbour tables and baselines (stdadk_knn_f32, stdadk_knn_apply_f32, stnf.utils.baselines) at their real shapes:
  shared   10 000 sites, 4 000 of them sources, leave-one-out, k = 8: one table for the whole grid
  pertime  the same with the sources drawn per time slice, 100 slices in one call
  raster   a 200 x 200 raster (k = 1) against 10 000 and 100 000 sites
  grid     grid_scores at 100 000 sites x 100 times (the C2 model) without the key and with `baselines: true` on
           site-wise masks (one shared table), and grid_baselines alone on per-entry masks for --pertime-slices slices
           (a search per slice)
Beside each search the same task by torch.cdist + topk on the device (what a user would write; the bytes of its distance
matrix are noted), by scipy.spatial.cKDTree and by knn_host (numpy float64) on the host of the same box, 16 threads at
the most.  Device time is HIP events around batches of calls, median; per kernel the library's own event profiler.
Every GPU step is a child process under its own time limit; the first one that fails ends the run.  One JSON line each.
usage (MI355X): python tools/bench_baselines.py [--reps 5] [--grid] [--only-grid-without-key]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--child", default="", help="run one step in this process: shared | pertime | raster | grid")
ap.add_argument("--grid", action="store_true", help="also time grid_scores with and without the key")
ap.add_argument("--grid-sites", type=int, default=100000)
ap.add_argument("--pertime-slices", type=int, default=10)
ap.add_argument("--only-grid-without-key", action="store_true",
                help="the grid child times grid_scores without the key only (runs on a tree without the feature too)")
args = ap.parse_args()
if not args.child:
    for what in ("shared", "pertime", "raster") + (("grid",) if args.grid else ()):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(args.reps), "--grid-sites",
               str(args.grid_sites), "--pertime-slices", str(args.pertime_slices)]
        subprocess.run(cmd + (["--only-grid-without-key"] if args.only_grid_without_key else []), check=True, timeout=420)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
torch.set_num_threads(min(16, torch.get_num_threads()))
from stnf.models import STInterpMLP

d = torch.device("cuda:0")
rs = np.random.RandomState(0)
CALLS = 3


def events(fn, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


if args.child == "grid":
    from stnf.utils import grid_scores
    S, T = args.grid_sites, 100
    torch.manual_seed(0)
    m = STInterpMLP(p=0, k_spatial_centers=[1024, 4096, 5184], k_temporal_centers=[10, 15, 45],
                    hidden_dims=[256, 256, 128], dropout=0.0).to(d).eval()
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = rs.standard_normal((T, S)).astype(np.float32)
    u = np.broadcast_to(rs.uniform(size=S), (T, S))              # site-wise splits: one shared table
    masks = [u < 0.85, (u >= 0.85) & (u < 0.92), u >= 0.92]
    out = {}
    for key in (False,) * 4 if args.only_grid_without_key else (False, True, False, True):
        config = {"baselines": True} if key else {}
        grid_scores(m, z[:2], coords, *[k[:2] for k in masks], config=config)      # warm-up
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grid_scores(m, z, coords, *masks, config=config)
            ts.append(time.perf_counter() - t0)
        out.setdefault("with_key" if key else "without_key", []).append(statistics.median(ts))
    res = {"grid_scores_seconds": out, "sites": S, "times": T, "reps": args.reps, "masks": "site-wise"}
    if not args.only_grid_without_key:
        from stnf.utils import baselines as BL
        n = args.pertime_slices
        v = rs.uniform(size=(n, S))
        per = [v < 0.85, (v >= 0.85) & (v < 0.92), v >= 0.92]
        BL.grid_baselines(z[:1], coords, *[k[:1] for k in per], device=d)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = BL.grid_baselines(z[:n], coords, *per, device=d)
        res["grid_baselines_per_time"] = {"slices": n, "seconds": time.perf_counter() - t0, "shared_table": got["shared_table"],
                                          "pairs": float(n) * S * 0.85 * S}
        t0 = time.perf_counter()
        got = BL.grid_baselines(z, coords, *masks, device=d)
        res["grid_baselines_shared"] = {"slices": T, "seconds": time.perf_counter() - t0, "shared_table": got["shared_table"]}
    print(json.dumps(res), flush=True)
    sys.exit(0)

from scipy.spatial import cKDTree
from stnf import _native as N
from stnf.utils import baselines as BL


def search_record(name, q, coords, src, k, exclude_self, host_slices=None, numpy_host=True):
    """One search shape: device ms per call and per kernel, pairs per second; cdist + topk; cKDTree; knn_host."""
    M, S = len(q), len(coords)
    nM = 1 if src is None else len(src)
    n_src = float(nM * S if src is None else int((src != 0).sum()))
    qt, ct = torch.from_numpy(q).to(d), torch.from_numpy(coords).to(d)
    st = None if src is None else torch.from_numpy(src).to(d)
    idx = torch.empty((nM, M, k), dtype=torch.int32, device=d)
    d2 = torch.empty((nM, M, k), dtype=torch.float64, device=d)
    ws = torch.empty(N.knn_workspace_bytes(M, S, nM, k) // 8, dtype=torch.float64, device=d)
    fn = lambda: N.knn(qt, ct, st, k, exclude_self, idx, d2, ws)      # noqa: E731
    fn()
    torch.cuda.synchronize()
    res = {"shape": name, "targets": M, "sites": S, "slices": nM, "k": k, "exclude_self": bool(exclude_self),
           "pairs": M * n_src, "pairs_walked": float(nM) * M * S, "workspace_MiB": ws.numel() * 8 / 2 ** 20,
           "ms_per_call": statistics.median(events(fn) for _ in range(args.reps))}
    N.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    res["kernel_ms"] = {name.split("<")[0]: ms for name, ms in N.profile_collect()}
    N.profile_enable(False)
    res["pairs_per_s"] = res["pairs"] / (res["ms_per_call"] * 1e-3)
    # what a user would write on the device: the float32 distance matrix of a slice and topk, slice by slice
    slices = range(nM if host_slices is None else min(nM, host_slices))
    sel = [np.arange(S) if src is None else np.nonzero(src[m])[0] for m in slices]
    sel_t = [torch.from_numpy(s).to(d) for s in sel]

    def cdist_topk():
        for s in sel_t:
            dist = torch.cdist(qt, ct[s])
            if exclude_self:
                dist[s, torch.arange(len(s), device=d)] = float("inf")
            dist.topk(min(k, len(s)), dim=1, largest=False)
    cdist_topk()
    torch.cuda.synchronize()
    res["cdist_topk"] = {"slices": len(sel), "ms": statistics.median(events(cdist_topk, 1) for _ in range(args.reps)),
                         "distance_matrix_MiB_per_slice": M * len(sel[0]) * 4 / 2 ** 20}

    def tree():
        for s in sel:
            cKDTree(coords[s].astype(np.float64)).query(q.astype(np.float64), k=k + 1 if exclude_self else k)
    res["ckdtree"] = {"slices": len(sel), "seconds": wall(tree, 1)}
    if not numpy_host:
        return res
    t0 = time.perf_counter()
    hi, hd = BL.knn_host(q, coords, None if src is None else src[:len(sel)], k, exclude_self)
    res["knn_host"] = {"slices": len(sel), "seconds": time.perf_counter() - t0,
                       "equals_device": bool(np.array_equal(hi, idx[:len(sel)].cpu().numpy())
                                             and np.array_equal(hd, d2[:len(sel)].cpu().numpy()))}
    return res


if args.child in ("shared", "pertime"):
    S, k = 10000, 8
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    if args.child == "shared":
        src = np.zeros((1, S), dtype=np.uint8)
        src[0, rs.choice(S, 4000, replace=False)] = 1
        res = search_record("shared", coords, coords, src, k, True)
        # the table applied to 100 slices
        z = torch.from_numpy(rs.standard_normal((100, S)).astype(np.float32)).to(d)
        it, dt = (torch.from_numpy(a).to(d) for a in BL.knn_host(coords, coords, src, k, True))
        near, idw = torch.empty((100, S), device=d), torch.empty((100, S), device=d)
        ap_fn = lambda: N.knn_apply(it, dt, k, z, 2, near, idw)      # noqa: E731
        ap_fn()
        torch.cuda.synchronize()
        res["apply_100_slices_ms"] = statistics.median(events(ap_fn) for _ in range(args.reps))
    else:
        src = (rs.uniform(size=(100, S)) < 0.4).astype(np.uint8)
        res = search_record("pertime", coords, coords, src, k, True, host_slices=5)
    print(json.dumps(res), flush=True)
else:
    x = np.linspace(0, 1, 200).astype(np.float32)
    xg, yg = np.meshgrid(x, x)
    nodes = np.stack([xg.reshape(-1), yg.reshape(-1)], axis=1)
    for S in (10000, 100000):
        coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
        res = search_record(f"raster_{S}", nodes, coords, None, 1, False, numpy_host=S == 10000)
        values = rs.standard_normal(S).astype(np.float32)
        res["rasterize_nearest_seconds"] = wall(lambda: BL.rasterize_nearest(coords, values, device=d), args.reps)
        print(json.dumps(res), flush=True)
