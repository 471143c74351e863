"""The gmm knot initialiser on the device against the host sklearn path, on the same machine:
  workload 1: the default levels [25, 81, 121] on 10 000 points = 500 sites with temporal duplicates;
  workload 2: one level of 1 024 components on the same points.
Host = SpatialBasisEmbedding(init_method='gmm') as it was before init_device existed (three GaussianMixture.fit calls);
device = the same constructor with init_device='cuda' (k-means++ seeding on the host, EM through stdadk_gmm_em_f64).
Then the split of one device iteration: the four kernels' device times (stdadk_profile_enable, HIP events around every
launch -- a run of its own, the events serialise the launches) beside the wall time per iteration of an unprofiled fit,
whose remainder is launch overhead plus the 8-byte read of the lower bound.
Every GPU step is a child process under its own time limit; the first one that fails ends the run.  Writes
profiles/gmm_init.md.      usage (MI355X): python tools/bench_gmm_init.py [--reps 3] [--out profiles/gmm_init.md]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"default": [25, 81, 121], "k1024": [1024]}
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm_init.md"))
ap.add_argument("--child", default="", help="run one workload in this process")
args = ap.parse_args()

if not args.child:
    rows = {}
    for name in WORKLOADS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps)],
                             check=True, timeout=540, capture_output=True, text=True).stdout
        rows[name] = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
        print(json.dumps(rows[name]), flush=True)
    md = ["# gmm knot initialiser: device against host", "",
          "`python tools/bench_gmm_init.py` on one MI355X box: 10 000 float64 points (500 sites with temporal duplicates),",
          "host = `SpatialBasisEmbedding(init_method='gmm')` (sklearn, the only path before `init_device`), device = the same",
          f"constructor with `init_device='cuda'`; medians of {args.reps} runs each, alternating; both give the same knots",
          "(largest difference in float32 ulps in the last column).", "",
          "| workload | levels | host s | device s | ratio | of it k-means++ seeding (host) s | EM iterations | ulps |",
          "|---|---|---|---|---|---|---|---|"]
    for name, r in rows.items():
        md.append(f"| {name} | {r['levels']} | {r['host_s']:.3f} | {r['device_s']:.4f} | {r['host_s'] / r['device_s']:.0f}x | "
                  f"{r['seeding_s']:.4f} | {r['iterations']} | {r['ulps']:.2f} |")
    md += ["", "What is left of the device path is the seeding, which stays sklearn's own `kmeans_plusplus` on the host so that",
           "the seeds are those of `GaussianMixture(random_state=42)`: " +
           "; ".join(f"{name}: {r['seeding_s'] / r['device_s']:.0%} of the device time, the EM itself "
                     f"{1e-3 * r['iterations'] * r['iter_wall_us']:.1f} ms against {r['host_s'] - r['seeding_s']:.2f} s of host EM "
                     f"({(r['host_s'] - r['seeding_s']) / (1e-6 * r['iterations'] * r['iter_wall_us']):.0f}x)"
                     for name, r in rows.items()) + "."]
    md += ["", "One EM iteration on the device (all restarts of all levels of the workload, per iteration):", "",
           "| workload | wall per iteration us | kernels us (profiled run) | lpn | sums | var | finish | launches + host read us |",
           "|---|---|---|---|---|---|---|---|"]
    for name, r in rows.items():
        k = r["kernel_us"]
        md.append(f"| {name} | {r['iter_wall_us']:.1f} | {sum(k.values()):.1f} | {k['gmm_lpn_kernel']:.1f} | "
                  f"{k['gmm_sums_kernel']:.1f} | {k['gmm_var_kernel']:.1f} | {k['gmm_finish_kernel']:.1f} | "
                  f"{r['iter_wall_us'] - sum(k.values()):.1f} |")
    md += ["", "The wall time per iteration is that of an unprofiled fit (EM only, seeding excluded); the kernel times come",
           "from a separate run with HIP events around every launch (the events lengthen a short kernel: the one-workgroup",
           "finish kernel does almost nothing).  The remainder is four launches and the blocking 8-byte read of the lower",
           "bound that the convergence test needs.", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(md))
    print("wrote", args.out)
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
from stnf import _native as N
from stnf import knot_init
from stnf.models.st_interp import SpatialBasisEmbedding

levels = WORKLOADS[args.child]
rs = np.random.RandomState(0)
sites = rs.uniform(0.0, 1.0, (500, 2))
coords = sites[rs.randint(0, 500, 10000)]
torch.zeros(1, device="cuda").item()                  # the HIP runtime is up before anything is timed


def build(device):
    np.random.seed(0)
    t0 = time.perf_counter()
    emb = SpatialBasisEmbedding(n_centers=levels, init_method='gmm', train_coords=coords, init_device=device)
    return time.perf_counter() - t0, emb


build("cuda")                                          # library load, first launches
host, dev = [], []
for _ in range(args.reps):
    t, e_dev = build("cuda")
    dev.append(t)
    t, e_host = build(None)
    host.append(t)
sp = lambda a, b: float((np.abs(a.double() - b.double()) / np.spacing(np.abs(b.numpy())).astype(np.float64)).max())  # noqa: E731
ulps = max(sp(e_dev.centers, e_host.centers), sp(e_dev.bandwidths, e_host.bandwidths))

# the pieces of the device path: seeding, then the fits alone (unprofiled wall, then kernel times under events)
t0 = time.perf_counter()
seeds = knot_init.kmeanspp_seeds(coords, levels)
seeding = time.perf_counter() - t0
pts = torch.from_numpy(coords).cuda()


def fits():
    return sum(sum(knot_init.fit_spherical_gmm(pts, k, s).n_iter) for k, s in zip(levels, seeds))


fits()
torch.cuda.synchronize()
t0 = time.perf_counter()
iters = fits()
torch.cuda.synchronize()
wall = time.perf_counter() - t0
N.profile_enable(True)
fits()
torch.cuda.synchronize()
recs = N.profile_collect()
N.profile_enable(False)
kern = {}
for name, ms in recs:
    kern[name] = kern.get(name, 0.0) + ms
print(json.dumps(dict(workload=args.child, levels=levels, host_s=statistics.median(host), device_s=statistics.median(dev),
                      seeding_s=seeding, iterations=iters, ulps=ulps, iter_wall_us=1e6 * wall / iters,
                      kernel_us={k: 1e3 * v / iters for k, v in kern.items()})))
