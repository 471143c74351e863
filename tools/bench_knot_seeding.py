"""k-means++ seeding of the gmm and kmeans_balanced knot initialisers: sklearn on the host (the parent's path, the
default) against stdadk_kmeanspp_f64 (seeding='device'), on the same box in alternating runs.
  seeding alone: knot_init.kmeanspp_seeds (host) against knot_init.kmeanspp_seeds_device (stream drawn on the host, one
                 call per level with the three restarts side by side, one read of the rows), points already on the device;
  whole constructor: SpatialBasisEmbedding(init_method='gmm', init_device='cuda') with init_seeding 'host' / 'device'.
Workloads: the default levels [25, 81, 121] on 10 000 points = 500 sites with temporal duplicates (the workload of
profiles/gmm_init.md); [1024] and the C2 levels [1024, 4096, 5184] on 10 000 distinct uniform points (more seeds than
distinct points would leave nothing to compare).  kmeans_balanced: default levels, whole constructor both ways, for the
share seeding has there.  Every device result is checked against the host's seeds in coordinates.
The GPU work is one child process under its own time limit.  Writes profiles/knot_seeding.md.
usage (MI355X): python tools/bench_knot_seeding.py [--reps 5] [--skip-kmeans] [--out profiles/knot_seeding.md]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT, ONE, C2 = [25, 81, 121], [1024], [1024, 4096, 5184]
MARK = "<!-- notes: kept by tools/bench_knot_seeding.py when it rewrites the tables above -->\n"
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-kmeans", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knot_seeding.md"))
ap.add_argument("--child", action="store_true", help="measure in this process")
args = ap.parse_args()

if not args.child:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)] + (["--skip-kmeans"] if args.skip_kmeans else [])
    out = subprocess.run(cmd, check=True, timeout=840, stdout=subprocess.PIPE, text=True).stdout
    r = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(r), flush=True)
    ms = lambda v: f"{1e3 * v['median']:.2f} ({1e3 * v['min']:.2f}-{1e3 * v['max']:.2f})"      # noqa: E731
    md = ["# k-means++ seeding of the knot initialisers: host against device", "",
          "`python tools/bench_knot_seeding.py` on one MI355X box, host and device runs alternating; milliseconds, median",
          "(min-max).  Host = `sklearn.cluster.kmeans_plusplus`, three restarts per level on one `RandomState(42)` (the",
          "parent's path and still the default).  Device = the same random stream drawn on the host, one",
          "`stdadk_kmeanspp_f64` call per level with the three restarts side by side, one read of the 3 k rows.", "",
          "| workload | levels | reps | seeding host | seeding device | host / device | kernel alone, per level | gmm constructor, host seeding | "
          "gmm constructor, device seeding | host / device | seeds equal in coordinates |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for w in r["workloads"]:
        md.append(f"| {w['points']} | {w['levels']} | {w['reps']} | {ms(w['seed_host'])} | {ms(w['seed_device'])} | "
                  f"{w['seed_host']['median'] / w['seed_device']['median']:.1f}x | {' + '.join(f'{v:.2f}' for v in w['kernel_ms'])} | {ms(w['gmm_host'])} | {ms(w['gmm_device'])} | "
                  f"{w['gmm_host']['median'] / w['gmm_device']['median']:.1f}x | {w['equal']} |")
    if r.get("kmeans"):
        k = r["kmeans"]
        md += ["", f"`kmeans_balanced`, levels {k['levels']}, {k['points']}: whole constructor {k['host_s']:.2f} s with host seeding, "
               f"{k['device_s']:.2f} s with device seeding (one run each); seeding alone is the first row above, "
               f"{100 * r['workloads'][0]['seed_host']['median'] / k['host_s']:.1f} % of the host-seeded constructor: the balancing "
               "kernel is what that initialiser costs, not the seeds.", ""]
    keep = ""                                          # what was written by hand below the marker stays
    if os.path.exists(args.out) and MARK in open(args.out).read():
        keep = MARK + open(args.out).read().split(MARK, 1)[1]
    with open(args.out, "w") as f:
        f.write("\n".join(md) + "\n" + keep)
    print("wrote", args.out)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
from stnf import _native as N
from stnf import knot_init
from stnf.models.st_interp import SpatialBasisEmbedding

rs = np.random.RandomState(0)
sites = rs.uniform(0.0, 1.0, (500, 2))
dup = sites[rs.randint(0, 500, 10000)]
distinct = np.random.RandomState(1).uniform(0.0, 1.0, (10000, 2))
torch.zeros(1, device="cuda").item()                  # the HIP runtime is up before anything is timed


def stats(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def build(method, coords, levels, seeding):
    np.random.seed(0)
    t0 = time.perf_counter()
    emb = SpatialBasisEmbedding(n_centers=levels, init_method=method, train_coords=coords, init_device="cuda",
                                init_seeding=seeding)
    return time.perf_counter() - t0, emb


def workload(name, coords, levels, reps):
    pts = torch.from_numpy(coords).cuda()
    knot_init.kmeanspp_seeds_device(pts, levels)                   # library load, first launch of this shape
    build("gmm", coords, levels, "device")
    t = dict(seed_host=[], seed_device=[], gmm_host=[], gmm_device=[])
    for _ in range(reps):
        t0 = time.perf_counter()
        host = knot_init.kmeanspp_seeds(coords, levels)
        t["seed_host"].append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = knot_init.kmeanspp_seeds_device(pts, levels)          # ends in the read of the rows
        t["seed_device"].append(time.perf_counter() - t0)
        dt, a = build("gmm", coords, levels, "host")
        t["gmm_host"].append(dt)
        dt, b = build("gmm", coords, levels, "device")
        t["gmm_device"].append(dt)
    kernel_ms = []                                                  # the launches alone, inputs staged, HIP events
    for k, (first, u) in zip(levels, knot_init.kmeanspp_stream(len(coords), levels)):
        fd, ud = torch.from_numpy(first).cuda(), torch.from_numpy(u).cuda()
        idx = torch.empty(knot_init.N_INIT, k, device="cuda", dtype=torch.int32)
        pot = torch.empty(knot_init.N_INIT, device="cuda", dtype=torch.float64)
        ws = torch.empty(N.kmeanspp_workspace_bytes(len(coords), k, knot_init.N_INIT) // 8, device="cuda", dtype=torch.float64)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(3):
            ev[0].record()
            N.kmeanspp(pts, fd, ud, idx, pot, ws)
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]))
        kernel_ms.append(statistics.median(ts))
    differ = [int((~(coords[np.stack(h)] == coords[np.stack(d)]).all(axis=-1)).sum()) for h, d in zip(host, dev)]
    equal = not any(differ)
    knots = bool(torch.equal(a.centers, b.centers) and torch.equal(a.bandwidths, b.bandwidths))
    out = dict(points=name, levels=levels, reps=reps, kernel_ms=kernel_ms, equal=f"{'yes' if equal else f'NO (seeds that differ, per level: {differ})'}; knots bit for bit: {'yes' if knots else 'NO'}",
               **{k: stats(v) for k, v in t.items()})
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


res = dict(workloads=[workload("10 000 points, 500 sites", dup, DEFAULT, args.reps),
                      workload("10 000 distinct points", distinct, DEFAULT, args.reps),
                      workload("10 000 distinct points", distinct, ONE, max(2, args.reps // 2)),
                      workload("10 000 distinct points", distinct, C2, 2)])
if not args.skip_kmeans:
    build("kmeans_balanced", dup[:2000], [25], "device")            # first launches of the balancing kernels
    res["kmeans"] = dict(levels=DEFAULT, points="10 000 points, 500 sites",
                         host_s=build("kmeans_balanced", dup, DEFAULT, "host")[0],
                         device_s=build("kmeans_balanced", dup, DEFAULT, "device")[0])
print(json.dumps(res))
