"""A/B of the delta-head training step (the configuration of the reference's Table 4.4: five quantile levels,
use_delta_reparameterization, non_crossing_lambda 1.0): one library call (TrainStep(fused_delta_step=True)) against the
five (fixed knots) or six (learnable knots) split calls, on bench.py's C2 model and the shipped YAML's shape (same
engine settings, data and pipelined step loop as its `timed()`), in 1 000-step windows.

    python tools/bench_delta_step.py                      # every configuration, fused and split alternating
    python tools/bench_delta_step.py --configs c2_fixed_4096 --launches
    python tools/bench_delta_step.py --other-tree DIR     # + the split path of another checkout (DIR/st-dadk_amd with
                                                          #   its library built), in processes of its own, alternating

One worker process per (tree, configuration): it builds one engine per mode, then alternates the modes window by
window (fused, split, fused, split ...), so that clock and box drift hit both alike.  Per mode it reports, over the
windows: the median and the spread of ms per step (wall clock around the loop and the final synchronize) and of the
HOST time per step (the loop alone, before the synchronize: what Python and the library's host code take to enqueue a
step).  --launches adds the launch list of one step per mode with per-launch event times (stdadk_profile_enable).
Prints one JSON object per worker."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C2 = dict(k_spatial_centers=[1024, 4096, 5184], k_temporal_centers=[10, 15, 45], hidden_dims=[256, 256, 128])
DAMP = dict(spatial_learnable=True, gradient_damping=True, damping_threshold=0.0, damping_strength=5.0)
TAUS = [0.05, 0.25, 0.5, 0.75, 0.95]
HEAD = dict(output_dim=5, use_delta_reparameterization=True)
LOSS = dict(loss="pinball", quantile_levels=TAUS, non_crossing_lambda=1.0)
# name -> (rows per step, model keywords, engine keywords, knot initialiser seed): the C2 model with fixed and with
# learnable knots at three batch sizes, and the shipped YAML's shape (227 scattered learnable knots, GMM initialiser)
CONFIGS = {
    "c2_fixed_4096": (4096, HEAD, LOSS, None),
    "c2_fixed_16384": (16384, HEAD, LOSS, None),
    "c2_fixed_65536": (65536, HEAD, LOSS, None),
    "c2_learn_4096": (4096, dict(DAMP, **HEAD), dict(LOSS, domain_penalty_weight=0.01), None),
    "c2_learn_16384": (16384, dict(DAMP, **HEAD), dict(LOSS, domain_penalty_weight=0.01), None),
    "c2_learn_65536": (65536, dict(DAMP, **HEAD), dict(LOSS, domain_penalty_weight=0.01), None),
    "shipped_yaml_227_gmm_delta5": (4096, dict(DAMP, k_spatial_centers=[25, 81, 121], spatial_init_method="gmm", **HEAD),
                                    dict(LOSS, domain_penalty_weight=0.01), 0),
}


def worker(args):
    pkg = os.path.join(args.tree, "st-dadk_amd")
    sys.path.insert(0, pkg)
    import numpy as np
    import torch
    from stnf import _native as N
    from stnf.engine import TrainStep
    from stnf.models import STInterpMLP
    dev = torch.device("cuda", 0)
    B, model_kw, eng_kw, init_seed = CONFIGS[args.config]
    # bench.py's synthetic field (synth): coords ~ U[0,1)^2, t = i/99, y = smooth field + noise; 100 000 rows resident
    g = torch.Generator().manual_seed(2025)
    n = 100_000
    coords = torch.rand(n, 2, generator=g)
    t = torch.randint(0, 100, (n, 1), generator=g).float() / 99.0
    y = (torch.sin(4 * np.pi * coords[:, :1]) * torch.cos(3 * np.pi * coords[:, 1:2])
         * (1 + 0.5 * torch.sin(2 * np.pi * t)) + 0.1 * torch.randn(n, 1, generator=g))
    coords, t, y = coords.to(dev), t.to(dev), y.to(dev)
    torch.manual_seed(0)
    perm = torch.randperm(n, device=dev)
    nb = max(n // B, 1)

    def sl(i):
        return perm[(i % nb) * B:(i % nb) * B + B]

    engines = {}
    for mode in args.modes.split(","):
        torch.manual_seed(0)
        mk = dict(C2, p=0, dropout=0.1, layernorm=True)
        mk.update(model_kw)
        if init_seed is not None:
            np.random.seed(init_seed)
            mk["train_coords"] = coords[:20000].cpu().numpy()
        m = STInterpMLP(**mk).to(dev).train()
        kw = dict(eng_kw)
        if mode == "fused":
            kw["fused_delta_step"] = True
        e = TrainStep(m, lr=2e-2, weight_decay=5e-4, grad_clip=10.0, ema_decay=0.999, max_batch=B, **kw)
        assert bool(getattr(e, "_delta_step", False)) == (mode == "fused") and not getattr(e, "_knot_step", False)
        for i in range(5):
            e.step_indexed(coords, t, y, sl(i), next_idx=sl(i + 1))
        torch.cuda.synchronize()
        engines[mode] = [e, 5]
    K = args.steps
    wall = {m: [] for m in engines}
    host = {m: [] for m in engines}
    for w in range(args.windows):
        for mode, st in engines.items():
            e, i0 = st
            t0 = time.perf_counter()
            for i in range(i0, i0 + K):
                e.step_indexed(coords, t, y, sl(i), next_idx=sl(i + 1))
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            st[1] = i0 + K
            wall[mode].append((t2 - t0) / K * 1e3)
            host[mode].append((t1 - t0) / K * 1e3)
    out = {"tree": args.label, "config": args.config, "rows": B, "steps_per_window": K, "modes": {}}
    for mode, (e, i0) in engines.items():
        r = {"path": "window" if e.uses_window else "materialised",
             "ms_per_step_median": round(statistics.median(wall[mode]), 5),
             "ms_per_step_windows": [round(x, 5) for x in wall[mode]],
             "obs_per_s_median": round(B / statistics.median(wall[mode]) * 1e3),
             "host_ms_per_step_median": round(statistics.median(host[mode]), 5),
             "host_ms_per_step_windows": [round(x, 5) for x in host[mode]],
             "loss_finite": bool(torch.isfinite(e.loss_sum).all().item())}
        if args.launches:
            # one step with every launch bracketed by events, then the same step again for the times of a warm launch
            for rep in range(2):
                torch.cuda.synchronize()
                N.profile_enable(True)
                try:
                    e.step_indexed(coords, t, y, sl(i0 + rep), next_idx=sl(i0 + rep + 1))
                    torch.cuda.synchronize()
                    lst = N.profile_collect()
                finally:
                    N.profile_enable(False)
            r["launches_us"] = [[k, round(ms * 1e3, 2)] for k, ms in lst]
            r["launches_sum_us"] = round(sum(ms for _, ms in lst) * 1e3, 2)
        out["modes"][mode] = r
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--steps", type=int, default=1000, help="steps per window")
    ap.add_argument("--windows", type=int, default=3, help="windows per mode, the modes alternating")
    ap.add_argument("--rounds", type=int, default=1, help="with --other-tree: worker processes per tree, alternating")
    ap.add_argument("--launches", action="store_true", help="add the launch list with per-launch event times")
    ap.add_argument("--other-tree", default=None, help="another checkout whose split path is measured beside this one's")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--config", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--modes", default="fused,split",
                    help="modes measured in this tree")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    for cfg in args.configs.split(","):
        if cfg not in CONFIGS:
            ap.error(f"unknown configuration {cfg}; one of {list(CONFIGS)}")
        trees = [("this", ROOT, args.modes)] + ([("other", os.path.abspath(args.other_tree), "split")]
                                                   if args.other_tree else [])
        for _ in range(args.rounds):
            for label, tree, modes in trees:
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--label", label, "--config",
                       cfg, "--modes", modes, "--steps", str(args.steps), "--windows", str(args.windows)]
                if args.launches:
                    cmd.append("--launches")
                env = dict(os.environ)
                env.pop("STNF_FUSED_KNOT_STEP", None)
                env.pop("STNF_FUSED_DELTA_STEP", None)
                r = subprocess.run(cmd, env=env, timeout=900)
                if r.returncode != 0:
                    # a worker that died may have faulted the device: nothing more is started on it
                    sys.exit(f"worker {label}/{cfg} ended with status {r.returncode}; stopping")


if __name__ == "__main__":
    main()
