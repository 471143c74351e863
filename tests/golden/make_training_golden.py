#!/usr/bin/env python3
"""Generate the train_model golden by running the REAL reference's `train_model` (scripts/train_st_interp.py:463-881)
with unshuffled loaders.  Runs only where /root/reference is on disk; the committed files hold data only:

  tests/golden/<case>.npz            per TRAIN_CASES entry: the `history` columns of the reference in float32 and in
                                     float64 (`model.double()`, float64 data), the learning rate of every parameter group
                                     at every optimiser step, and (learnable knots) the initial knot tensors
  tests/golden/sched_*.npz           per SCHED_CASES entry: the per-step rates and the lr column of a longer schedule
  tests/golden/training_achieved.json  per case, history column and epoch: |float32 - float64| of the reference itself,
                                     the yardstick of tests/test_gpu_training_golden.py

Both branches of the reference run in double as they are (no substitute needed).  The loaders are lists of dict
batches in index order (what `DataLoader(shuffle=False)` with the reference's `collate_fn` yields); dropout is 0.

    python tests/golden/make_training_golden.py
"""
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")
sys.path.insert(0, "/root/reference/scripts")

import cases  # noqa: E402
import training_cases as tc  # noqa: E402
import train_st_interp as ref  # noqa: E402
from stnf.models.st_interp import STInterpMLP  # noqa: E402

torch.set_num_threads(8)
COLUMNS = ("train_loss", "val_loss", "val_rmse", "lr")


def build(case, dtype):
    cfg = tc.model_cfg(case)
    kn = case.get("knots", {})
    m = STInterpMLP(p=cfg["p"], k_spatial_centers=cfg["k_spatial_centers"],
                    k_temporal_centers=cfg["k_temporal_centers"], hidden_dims=cfg["hidden_dims"], dropout=0.0,
                    layernorm=cfg["layernorm"], spatial_learnable=case["learnable"], spatial_init_method="uniform",
                    spatial_basis_function=cfg["basis"], output_dim=cfg["output_dim"],
                    gradient_damping=kn.get("gradient_damping", False),
                    damping_threshold=kn.get("damping_threshold", 0.3),
                    damping_strength=kn.get("damping_strength", 1.0))
    st = cases.make_state(cfg)
    sd = m.state_dict()
    for k, v in st.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v.copy())
    m.load_state_dict(sd)
    return m.to(dtype)


def loader(arrays, batch, dtype):
    X, coords, t, y = (torch.from_numpy(a).to(dtype) for a in arrays)
    n = coords.shape[0]
    return [{"X": X[s:s + batch], "coords": coords[s:s + batch], "t": t[s:s + batch], "y": y[s:s + batch]}
            for s in range(0, n, batch)]


def run(case, rows, val_rows, dtype):
    """The reference's train_model; returns (history, per-step rates [steps, groups])."""
    tr, va = tc.data(case, rows, val_rows)
    batch = case["config"]["batch_size"]
    model = build(case, dtype)
    rates = []

    class Recording(torch.optim.AdamW):
        def step(self, *a, **kw):
            rates.append([float(g["lr"]) for g in self.param_groups])
            return super().step(*a, **kw)

    real = ref.optim.AdamW
    ref.optim.AdamW = Recording
    try:
        with tempfile.TemporaryDirectory() as tmp:
            _, hist, _ = ref.train_model(model, loader(tr, batch, dtype), loader(va, batch, dtype),
                                         dict(case["config"]), torch.device("cpu"), Path(tmp))
    finally:
        ref.optim.AdamW = real
    return {k: np.asarray([float(v) for v in hist[k]], np.float64) for k in COLUMNS}, np.asarray(rates, np.float64)


def main():
    achieved = {}
    for name, case in tc.TRAIN_CASES.items():
        h32, r32 = run(case, tc.TRAIN_ROWS, tc.VAL_ROWS, torch.float32)
        h64, r64 = run(case, tc.TRAIN_ROWS, tc.VAL_ROWS, torch.float64)
        assert np.array_equal(r32, r64) and np.array_equal(h32["lr"], h64["lr"])      # host arithmetic
        out = {f"h32/{k}": v for k, v in h32.items()}
        out.update({f"h64/{k}": v for k, v in h64.items()})
        out["rates"] = r64
        if case["learnable"]:
            sb = build(case, torch.float32).spatial_basis
            out["in_centers"] = sb.centers.detach().numpy().copy()
            out["in_log_bw"] = sb.log_bandwidths.detach().numpy().copy()
        np.savez(os.path.join(HERE, name + ".npz"), **out)
        achieved[name] = {k: [abs(float(a) - float(b)) for a, b in zip(h32[k], h64[k])] for k in COLUMNS}
        print(name, {k: (h64[k].tolist(), achieved[name][k]) for k in COLUMNS})
    for name, case in tc.SCHED_CASES.items():
        h, r = run(case, tc.SCHED_ROWS, tc.SCHED_VAL_ROWS, torch.float32)
        np.savez(os.path.join(HERE, name + ".npz"), lr=h["lr"], rates=r)
        print(name, r.shape, h["lr"].tolist())
    with open(os.path.join(HERE, "training_achieved.json"), "w") as f:
        json.dump({"what": "|reference float32 - reference float64| per history column and epoch "
                           "(make_training_golden.py)", "cases": achieved}, f, indent=1)


if __name__ == "__main__":
    main()
