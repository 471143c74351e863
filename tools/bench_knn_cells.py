"""The cell-binned neighbour search (stdadk_knn_cells_f32) against the brute-force one (stdadk_knn_f32), same process,
alternating, HIP events around three calls, median of three; the two tables compared for equality at every shape:
  shared        10 000 sites, 4 000 of them sources, leave-one-out, k = 8 (one shared table)
  pertime       the same with the sources drawn per time slice, 100 slices in one call
  raster_10000  a 200 x 200 raster (k = 1) against 10 000 sites; raster_100000 against 100 000
  pertime_100k  10 slices of 100 000 sites, 85 % of them sources, leave-one-out, k = 8
  clustered_100k  the same sizes, the sites in five tight clusters, every site a source, one slice
  sparse_100k   the same sizes, 2 % of the sites sources, 10 slices
then (--grid) grid_baselines as a whole on per-entry masks at 10 000 sites x 100 slices and 100 000 sites x 10 slices
with `baseline_search` "brute" and "cells" alternating, wall seconds, median of three.
--pairs (no GPU): the (target, source) pairs the plan meets at each shape, by the python restatement of
tests/golden/knn_cells_cases.py on ONE slice, beside targets x sources of that slice.
One JSON line each.  usage (MI355X): python tools/bench_knn_cells.py [--reps 3] [--grid] [--shapes a,b]
       (anywhere):   python tools/bench_knn_cells.py --pairs [--shapes a,b]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("shared", "pertime", "raster_10000", "raster_100000", "pertime_100k", "clustered_100k", "sparse_100k")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--grid", action="store_true", help="also time grid_baselines on per-entry masks with both searches")
ap.add_argument("--pairs", action="store_true", help="count the pairs the plan meets, on the host, and stop")
args = ap.parse_args()

import numpy as np
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))


def shape(name):
    """(q, coords, src, k, exclude_self) of a named shape, from its own seed."""
    rs = np.random.RandomState(SHAPES.index(name))
    if name.startswith("raster"):
        S = int(name.split("_")[1])
        x = np.linspace(0, 1, 200).astype(np.float32)
        xg, yg = np.meshgrid(x, x)
        return np.stack([xg.reshape(-1), yg.reshape(-1)], axis=1), rs.uniform(0, 1, (S, 2)).astype(np.float32), None, 1, False
    S = 10000 if name in ("shared", "pertime") else 100000
    if name == "clustered_100k":
        centres = rs.uniform(0.1, 0.9, (5, 2))
        coords = (centres[rs.randint(5, size=S)] + 0.01 * rs.standard_normal((S, 2))).astype(np.float32)
        return coords, coords, None, 8, True
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    if name == "shared":
        src = np.zeros((1, S), dtype=np.uint8)
        src[0, rs.choice(S, 4000, replace=False)] = 1
    else:
        nM, density = {"pertime": (100, 0.4), "pertime_100k": (10, 0.85), "sparse_100k": (10, 0.02)}[name]
        src = (rs.uniform(size=(nM, S)) < density).astype(np.uint8)
    return coords, coords, src, 8, True


if args.pairs:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from golden import knn_cells_cases as cc
    for name in args.shapes.split(","):
        q, coords, src, k, ex = shape(name)
        one = None if src is None else src[:1]
        t0 = time.perf_counter()
        met = cc.restate_cells(dict(q=q, coords=coords, src=one, k=k, exclude_self=ex))[2]
        brute = len(q) * (len(coords) if one is None else int((one != 0).sum()))
        print(json.dumps({"shape": name, "slice": 0, "grid_side": cc.grid_side(len(coords)), "pairs_met": int(met),
                          "pairs_brute": int(brute), "fraction": met / brute, "host_seconds": time.perf_counter() - t0}), flush=True)
    sys.exit(0)

import torch
torch.set_num_threads(min(16, torch.get_num_threads()))
from stnf import _native as N
from stnf.utils import baselines as BL

d = torch.device("cuda:0")
CALLS = 3


def events(fn, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


for name in args.shapes.split(","):
    q, coords, src, k, ex = shape(name)
    M, S = len(q), len(coords)
    nM = 1 if src is None else len(src)
    qt, ct = torch.from_numpy(q).to(d), torch.from_numpy(coords).to(d)
    st = None if src is None else torch.from_numpy(src).to(d)
    out, fns, ws_bytes = {}, {}, {}
    for search, sizer, call in (("brute", N.knn_workspace_bytes, N.knn), ("cells", N.knn_cells_workspace_bytes, N.knn_cells)):
        idx = torch.empty((nM, M, k), dtype=torch.int32, device=d)
        d2 = torch.empty((nM, M, k), dtype=torch.float64, device=d)
        ws = torch.empty(sizer(M, S, nM, k) // 8, dtype=torch.float64, device=d)
        out[search], ws_bytes[search] = (idx, d2), ws.numel() * 8
        fns[search] = (lambda call=call, idx=idx, d2=d2, ws=ws: call(qt, ct, st, k, ex, idx, d2, ws))
        fns[search]()
    torch.cuda.synchronize()
    ms = {"brute": [], "cells": []}
    for _ in range(args.reps):                                   # alternating
        for search in ("brute", "cells"):
            ms[search].append(events(fns[search]))
    res = {"shape": name, "targets": M, "sites": S, "slices": nM, "k": k, "exclude_self": ex,
           "pairs": float(M) * (nM * S if src is None else int((src != 0).sum())),
           "ms_per_call": {s: statistics.median(v) for s, v in ms.items()}, "ms_all": ms,
           "workspace_MiB": {s: b / 2 ** 20 for s, b in ws_bytes.items()},
           "tables_equal": bool(torch.equal(out["brute"][0], out["cells"][0])
                                and torch.equal(out["brute"][1].view(torch.int64), out["cells"][1].view(torch.int64)))}
    res["speedup"] = res["ms_per_call"]["brute"] / res["ms_per_call"]["cells"]
    N.profile_enable(True)
    fns["cells"]()
    torch.cuda.synchronize()
    res["cells_kernel_ms"] = {n.split("<")[0]: ms_ for n, ms_ in N.profile_collect()}
    N.profile_enable(False)
    print(json.dumps(res), flush=True)

if args.grid:
    for S, T in ((10000, 100), (100000, 10)):
        rs = np.random.RandomState(S)
        coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
        z = rs.standard_normal((T, S)).astype(np.float32)
        v = rs.uniform(size=(T, S))
        masks = [v < 0.85, (v >= 0.85) & (v < 0.92), v >= 0.92]
        got, secs = {}, {"brute": [], "cells": []}
        for search in ("brute", "cells"):
            BL.grid_baselines(z[:1], coords, *[m[:1] for m in masks], config={"baseline_search": search}, device=d)
        for _ in range(args.reps):                               # alternating
            for search in ("brute", "cells"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[search] = BL.grid_baselines(z, coords, *masks, config={"baseline_search": search}, device=d)
                secs[search].append(time.perf_counter() - t0)
        same = True
        try:
            np.testing.assert_equal(got["cells"], got["brute"])
        except AssertionError:
            same = False
        print(json.dumps({"grid_baselines_per_time": {"sites": S, "slices": T, "shared_table": got["cells"]["shared_table"],
                                                      "seconds": {s: statistics.median(t) for s, t in secs.items()},
                                                      "seconds_all": secs, "results_equal": same}}), flush=True)
