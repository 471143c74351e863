"""The kmeans_balanced knot initialiser on the device, level by level, on 10 000 points = 800 sites with temporal
duplicates, the sites weighted towards one corner of the square (what the driver feeds the initialiser: one row per
observation), levels [25, 81, 121].  Per level: seconds of the fit (three restarts), iterations, unit augmentations per
iteration, and the share of the wall time the kernels take (stdadk_profile_enable: HIP events around every launch, a
run of its own) with the balancing kernel apart.  Beside them, on the same box: the whole constructor with
init_method='kmeans_balanced' and with init_method='gmm' (both init_device='cuda'), and the tests' numpy restatement
(tests/golden/kmeans_cases.py) on the host, seconds per iteration over the first iterations of the first restart.
The GPU work is one child process under its own time limit.  Writes profiles/kmeans_balanced.md.
usage (MI355X): python tools/bench_kmeans_init.py [--host-iters 3] [--out profiles/kmeans_balanced.md]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [25, 81, 121]
MARK = "<!-- notes: kept by tools/bench_kmeans_init.py when it rewrites the tables above -->\n"
ap = argparse.ArgumentParser()
ap.add_argument("--host-iters", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_balanced.md"))
ap.add_argument("--child", action="store_true", help="measure in this process")
args = ap.parse_args()

if not args.child:
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--host-iters", str(args.host_iters)],
                         check=True, timeout=900, stdout=subprocess.PIPE, text=True).stdout
    r = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(r), flush=True)
    md = ["# kmeans_balanced knot initialiser on the device", "",
          "`python tools/bench_kmeans_init.py` on one MI355X box: 10 000 float64 points (800 sites with temporal duplicates,",
          "weighted towards one corner), three k-means++ restarts per level, every iteration one",
          "`stdadk_kmeans_balanced_iter_f64` call (exact constrained assignment by successive shortest paths, one unit per",
          "path, inside one launch).  Nobody had measured this before; no time was set in advance.", "",
          "| k | lo-hi | fit s | seeding (host) s | iterations per restart | augmentations per iteration: first / median / last | "
          "wall per iteration ms | kernels ms | of it km_balance ms | kernels' share | host restatement s per iteration |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for L in r["levels"]:
        md.append(f"| {L['k']} | {L['lo']}-{L['hi']} | {L['fit_s']:.3f} | {L['seeding_s']:.3f} | {L['n_iter']} | "
                  f"{L['aug_first']} / {L['aug_median']:.0f} / {L['aug_last']} | {L['iter_wall_ms']:.2f} | {L['kernels_ms']:.2f} | "
                  f"{L['balance_ms']:.2f} | {L['kernels_ms'] / L['iter_wall_ms']:.0%} | {L['host_iter_s']:.2f} |")
    md += ["", f"Whole constructor, `init_device='cuda'`, levels {LEVELS}: kmeans_balanced {r['module_kmeans_s']:.2f} s, gmm "
           f"{r['module_gmm_s']:.3f} s (median of {r['reps']}).  Augmentations are those of the restart that was kept (first "
           "/ median / last iteration); the wall time per iteration is that of an unprofiled fit, the kernel times come from a "
           "profiled run and are per iteration over all restarts of the level.  The host restatement is the numpy "
           f"statement the tests compare against, over the first {r['host_iters']} iterations of the first restart.", ""]
    keep = ""                                          # what was written by hand below the marker stays
    if os.path.exists(args.out) and MARK in open(args.out).read():
        keep = MARK + open(args.out).read().split(MARK, 1)[1]
    with open(args.out, "w") as f:
        f.write("\n".join(md) + keep)
    print("wrote", args.out)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from golden import kmeans_cases as kc
from stnf import _native as N
from stnf import knot_init
from stnf.models.st_interp import SpatialBasisEmbedding

rs = np.random.RandomState(0)
sites = rs.uniform(0.0, 1.0, (800, 2))
weight = np.exp(-3.0 * (sites[:, 0] + sites[:, 1]))                 # denser towards the corner (0, 0)
coords = sites[rs.choice(800, 10000, p=weight / weight.sum())]
torch.zeros(1, device="cuda").item()                  # the HIP runtime is up before anything is timed
pts = torch.from_numpy(coords).cuda()
REPS = 3


def build(method):
    np.random.seed(0)
    t0 = time.perf_counter()
    SpatialBasisEmbedding(n_centers=LEVELS, init_method=method, train_coords=coords, init_device="cuda")
    return time.perf_counter() - t0


levels = []
for k in LEVELS:
    lo, hi = knot_init.balanced_bounds(len(coords), k)
    t0 = time.perf_counter()
    seeds = knot_init.kmeanspp_seeds(coords, [k])[0]
    seeding = time.perf_counter() - t0
    history = []
    if k == LEVELS[0]:
        knot_init.fit_balanced_kmeans(pts, k, seeds[:1], max_iter=2)          # library load, first launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = knot_init.fit_balanced_kmeans(pts, k, seeds, history=history)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    iters = sum(fit.n_iter)
    N.profile_enable(True)
    knot_init.fit_balanced_kmeans(pts, k, seeds)
    torch.cuda.synchronize()
    kern = {}
    for name, ms in N.profile_collect():
        kern[name] = kern.get(name, 0.0) + ms
    N.profile_enable(False)
    aug = [h[2] for h in history[fit.best]]
    mu, t0 = coords[np.asarray(seeds[0], np.int64)].copy(), time.perf_counter()
    for _ in range(args.host_iters):
        mu = kc.iteration(coords, mu, lo, hi)["mu"]
    host_iter = (time.perf_counter() - t0) / args.host_iters
    levels.append(dict(k=k, lo=lo, hi=hi, fit_s=wall, seeding_s=seeding, n_iter=fit.n_iter, aug_first=aug[0],
                       aug_median=statistics.median(aug), aug_last=aug[-1], iter_wall_ms=1e3 * wall / iters,
                       kernels_ms=sum(kern.values()) / iters, balance_ms=kern["km_balance_kernel"] / iters,
                       host_iter_s=host_iter, inertia=fit.inertia))
    print(json.dumps(levels[-1]), file=sys.stderr, flush=True)
build("gmm")                                            # first launches of the gmm kernels; the fits above warmed the others
module = {m: statistics.median(build(m) for _ in range(REPS)) for m in ("kmeans_balanced", "gmm")}
print(json.dumps(dict(levels=levels, module_kmeans_s=module["kmeans_balanced"], module_gmm_s=module["gmm"], reps=REPS,
                      host_iters=args.host_iters)))
