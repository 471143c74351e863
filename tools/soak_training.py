"""End-to-end soak: KAUST-shaped synthetic field (S sites x T times, z = smooth field + N(0, 0.1^2) noise, 10 % held
out), C2 model, the reference's optimiser settings with a cosine learning-rate schedule: `stnf.training.train_model`
(run_epoch + validation under the EMA weights every epoch) over a device-resident dataset.  Prints the driver's line per
epoch, the best held-out RMSE and the rate; then the shipped multi-quantile shape on plain run_epoch.
`--checkpoint PATH` saves the run there at the end of every `--checkpoint-every`-th epoch (default 1) and times one save
at the end; `--resume` continues from that file when it exists.
usage (MI355X box): python tools/soak_training.py [epochs] [--checkpoint PATH [--checkpoint-every K] [--resume]]"""
import argparse, math, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-dadk_amd"))
from stnf.models import STInterpMLP
from stnf.engine import TrainStep
from stnf.training import train_model, evaluate_model, make_engine
from stnf.checkpoint import save_checkpoint
from stnf.dataio.device_dataset import DeviceDataset
from stnf.utils import set_seed

ap = argparse.ArgumentParser()
ap.add_argument("epochs", nargs="?", type=int, default=60)
ap.add_argument("--checkpoint", default=None)
ap.add_argument("--checkpoint-every", type=int, default=1)
ap.add_argument("--resume", action="store_true")
args = ap.parse_args()
epochs = args.epochs
set_seed(0)
rs = np.random.RandomState(0)
S, T = 2000, 100
coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
tt = np.arange(T) / (T - 1)
field = (np.sin(4 * np.pi * coords[None, :, 0]) * np.cos(3 * np.pi * coords[None, :, 1])
         * (1 + 0.5 * np.sin(2 * np.pi * tt[:, None])))
z = (field + 0.1 * rs.standard_normal((T, S))).astype(np.float32)
mask = rs.uniform(size=(T, S)) < 0.9                       # 90 % train, 10 % held out
ds = DeviceDataset.from_mask(z, coords, mask)
dv = DeviceDataset.from_mask(z, coords, ~mask)
clean = DeviceDataset.from_mask(field.astype(np.float32), coords, ~mask)
d = torch.device("cuda:0")
m = STInterpMLP(p=0, k_spatial_centers=[1024, 4096, 5184], k_temporal_centers=[10, 15, 45], hidden_dims=[256, 256, 128],
                dropout=0.1, layernorm=True).to(d)
B = 4096
nb = math.ceil(len(ds) / B)
config = {"lr": 2e-2, "weight_decay": 5e-4, "grad_clip": 10.0, "batch_size": B, "epochs": epochs, "scheduler": "cosine",
          "patience": epochs + 1}
g = torch.Generator(device=d).manual_seed(0)
eng = make_engine(m, config, B, nb)
t0 = time.perf_counter()
m, hist, _ = train_model(m, ds, dv, config, generator=g, engine=eng,     # validation under EMA after every epoch
                         checkpoint=args.checkpoint, checkpoint_every=args.checkpoint_every, resume=args.resume)
torch.cuda.synchronize()
el = time.perf_counter() - t0
print(f"epoch time incl. validation{' and checkpoints' if args.checkpoint else ''}: {1e3 * el / epochs:.2f} ms "
      f"(wall time of this call / {epochs} epochs)")
if args.checkpoint:
    saves = []
    for _ in range(5):
        t1 = time.perf_counter()
        save_checkpoint(args.checkpoint + ".probe", eng)
        saves.append(1e3 * (time.perf_counter() - t1))
    probe_size = os.path.getsize(args.checkpoint + ".probe")
    os.remove(args.checkpoint + ".probe")
    print(f"one save of the engine's state alone (file of {probe_size / 2 ** 20:.1f} MiB): "
          f"{sorted(saves)[2]:.1f} ms (median of 5: {', '.join(f'{s:.1f}' for s in saves)}); the driver's file, with "
          f"its best state: {os.path.getsize(args.checkpoint) / 2 ** 20:.1f} MiB")
rmse_clean = evaluate_model(m, clean, config)["rmse"]               # the returned model holds the best EMA state
assert all(math.isfinite(v) for v in hist["train_loss"] + hist["val_rmse"])
print(f"best held-out RMSE vs noisy {min(hist['val_rmse']):.4f} (noise floor 0.1000)  vs the noise-free field {rmse_clean:.4f}")
print(f"{epochs} epochs x {nb} steps of {B} in {el:.2f} s incl. validation every epoch = {epochs * len(ds) / el / 1e6:.1f} M obs/s end to end")


# ---- the shipped configuration's shape: 227 GMM-initialised learnable knots, 5 quantiles, non-crossing penalty
taus = [0.05, 0.25, 0.5, 0.75, 0.95]
np.random.seed(0)
m2 = STInterpMLP(p=0, k_spatial_centers=[25, 81, 121], k_temporal_centers=[10, 15, 45], hidden_dims=[256, 256, 128],
                 dropout=0.1, layernorm=True, spatial_learnable=True, spatial_init_method="gmm", train_coords=coords,
                 gradient_damping=True, damping_threshold=0.0, damping_strength=5.0, output_dim=5).to(d)
m2.train()
e2 = TrainStep(m2, lr=2e-2, weight_decay=5e-4, grad_clip=10.0, ema_decay=1.0 - 1.0 / (10.0 * nb), max_batch=B,
               loss="pinball", quantile_levels=taus, non_crossing_weight=0.5, domain_penalty_weight=0.01)
c0 = m2.spatial_basis.centers.detach().clone()
t0 = time.perf_counter()
for ep in range(epochs):
    e2.set_lr(2e-2 * 0.5 * (1 + math.cos(math.pi * ep / epochs)))
    e2.set_basis_lr(0.05 * 2e-2 * 0.5 * (1 + math.cos(math.pi * ep / epochs)))
    tr = e2.run_epoch(ds, B, generator=g)
torch.cuda.synchronize()
el = time.perf_counter() - t0
e2.swap_in_ema()
m2.eval()
with torch.no_grad():
    pq = m2(None, dv.coords, dv.t.view(-1, 1))
cover = [(float((dv.y[:, 0] <= pq[:, i]).float().mean())) for i in range(5)]
cross = float((pq[:, 1:] < pq[:, :-1]).float().mean())
moved = float((m2.spatial_basis.centers.detach() - c0).norm(dim=1).mean())
print(f"multi-quantile + learnable knots: objective {tr:.5f}; held-out coverage P(y <= q_tau) for tau {taus}: "
      f"{[round(c, 3) for c in cover]}; crossing fraction {cross:.4f}; mean knot displacement {moved:.4f}; "
      f"{epochs * len(ds) / el / 1e6:.1f} M obs/s")
assert all(math.isfinite(c) for c in cover) and math.isfinite(tr)
