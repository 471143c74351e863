"""Validation pass under EMA weights, C2 model, 100 000 rows in batches of 65 536: the swap way (swap_in_ema + Predictor
+ torch metrics + second swap, what tools/soak_training.py did before stnf.training existed) against
Evaluator.evaluate(params="ema"), alternating, medians; then train_model's end-to-end rate (validation every epoch) on
the soak set beside the pure run_epoch rate.  Prints one JSON line.
usage (MI355X): python tools/bench_validation.py [--reps 15] [--epochs 10] [--only-eval]
(kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_validation.py --only-eval`)"""
import argparse, json, math, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
from stnf.models import STInterpMLP
from stnf.engine import TrainStep, Predictor
from stnf.evaluation import Evaluator
from stnf.dataio.device_dataset import DeviceDataset
from stnf import training as T

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--epochs", type=int, default=10)
ap.add_argument("--only-eval", action="store_true")
args = ap.parse_args()
d = torch.device("cuda:0")
torch.manual_seed(0)


def c2():
    return STInterpMLP(p=0, k_spatial_centers=[1024, 4096, 5184], k_temporal_centers=[10, 15, 45],
                       hidden_dims=[256, 256, 128], dropout=0.1, layernorm=True).to(d).train()


def rows(n, seed):
    g = torch.Generator(device=d).manual_seed(seed)
    c = torch.rand(n, 2, device=d, generator=g)
    t = torch.rand(n, 1, device=d, generator=g)
    y = torch.sin(4 * math.pi * c[:, :1]) * torch.cos(3 * math.pi * c[:, 1:]) + 0.1 * torch.randn(n, 1, device=d, generator=g)
    return DeviceDataset(c, t, y)


m = c2()
eng = TrainStep(m, lr=2e-2, weight_decay=5e-4, grad_clip=10.0, ema_decay=0.99, max_batch=4096)
tr, va = rows(40960, 1), rows(100000, 2)
eng.run_epoch(tr, 4096)
VB = 65536
pred = Predictor(m, chunk=VB)
ev = Evaluator(m, max_batch=VB)


def swap_way():
    """2 host syncs (.item() per number), as the soak script read them"""
    eng.swap_in_ema()
    m.eval()
    p = pred.predict(va.coords, va.t)
    m.train()
    eng.swap_in_ema()
    return float(((p - va.y) ** 2).mean()), float((p - va.y).abs().mean())


def new_way():
    r = ev.evaluate(va, VB, params="ema", engine=eng)           # 1 host sync
    return r["mse"], r["mae"]


a, b = swap_way(), new_way()
assert abs(a[0] - b[0]) <= 1e-5 * a[0] and abs(a[1] - b[1]) <= 1e-5 * a[1], (a, b)
ts = {"swap": [], "evaluator": []}
for _ in range(args.reps):
    for name, fn in (("swap", swap_way), ("evaluator", new_way)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts[name].append((time.perf_counter() - t0) * 1e3)
out = {"rows": len(va), "batch": VB, "swap_ms": statistics.median(ts["swap"]),
       "evaluator_ms": statistics.median(ts["evaluator"]), "swap_ms_all": [round(x, 3) for x in ts["swap"]],
       "evaluator_ms_all": [round(x, 3) for x in ts["evaluator"]], "host_syncs": {"swap": 2, "evaluator": 1}}
out["ratio_swap_over_evaluator"] = out["swap_ms"] / out["evaluator_ms"]

if not args.only_eval:
    # the soak set (tools/soak_training.py): 2000 sites x 100 times, 90 % train / 10 % held out, B = 4096
    rs = np.random.RandomState(0)
    S, Tn = 2000, 100
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    tt = np.arange(Tn) / (Tn - 1)
    z = (np.sin(4 * np.pi * coords[None, :, 0]) * np.cos(3 * np.pi * coords[None, :, 1])
         * (1 + 0.5 * np.sin(2 * np.pi * tt[:, None])) + 0.1 * rs.standard_normal((Tn, S))).astype(np.float32)
    mask = rs.uniform(size=(Tn, S)) < 0.9
    ds, dv = DeviceDataset.from_mask(z, coords, mask), DeviceDataset.from_mask(z, coords, ~mask)
    cfg = {"lr": 2e-2, "weight_decay": 5e-4, "grad_clip": 10.0, "batch_size": 4096, "epochs": args.epochs,
           "scheduler": "cosine", "patience": 10 ** 6, "verbose": False}
    g = torch.Generator(device=d).manual_seed(0)
    m1 = c2()
    T.train_model(m1, ds, dv, dict(cfg, epochs=2), generator=g)              # warm: code objects, allocator
    m1 = c2()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T.train_model(m1, ds, dv, cfg, generator=g)
    torch.cuda.synchronize()
    e2e = args.epochs * len(ds) / (time.perf_counter() - t0)
    m2 = c2()
    e2 = TrainStep(m2, lr=2e-2, weight_decay=5e-4, grad_clip=10.0, ema_decay=0.99, max_batch=4096)
    e2.run_epoch(ds, 4096, generator=g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.epochs):
        e2.run_epoch(ds, 4096, generator=g)
    torch.cuda.synchronize()
    pure = args.epochs * len(ds) / (time.perf_counter() - t0)
    out.update(train_rows=len(ds), val_rows=len(dv), epochs=args.epochs, train_model_rows_per_s=e2e,
               run_epoch_rows_per_s=pure)
print(json.dumps(out))
