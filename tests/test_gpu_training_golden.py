"""stnf.training.train_model against the reference's own train_model (tests/golden/make_training_golden.py): 3 epochs,
warm-up 1, dropout 0, unshuffled, ragged last batch, for fixed knots + MSE and for the shipped shape (learnable knots,
5 quantiles, non-crossing weight, progressive unfreezing).

Bound, per history column and epoch: the engine's distance to the reference's FLOAT64 history is at most 4 x the
reference-float32's distance to the same float64 history (tests/golden/training_achieved.json), with the project's
1e-5 relative as a floor -- both are independent float32 roundings of an amplifying AdamW recurrence.  The lr column is
host arithmetic: equal to 1e-12.  The reloaded best state equals the device-side best EMA copy bitwise.

Measured on MI355X, |engine - float64| / bound, worst over columns and epochs: 0.045 (fixed knots + MSE), 0.556
(learnable knots + 5 quantiles: val_loss of the second epoch, where the 1e-5 floor binds); every figure is printed."""
import json
import math
import os

import numpy as np
import pytest
import torch

from golden import cases
from golden import training_cases as tc
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(case, g):
    from stnf.models import STInterpMLP
    cfg = tc.model_cfg(case)
    kn = case.get("knots", {})
    m = STInterpMLP(p=cfg["p"], k_spatial_centers=cfg["k_spatial_centers"],
                    k_temporal_centers=cfg["k_temporal_centers"], hidden_dims=cfg["hidden_dims"], dropout=0.0,
                    layernorm=cfg["layernorm"], spatial_learnable=case["learnable"],
                    spatial_basis_function=cfg["basis"], output_dim=cfg["output_dim"],
                    gradient_damping=kn.get("gradient_damping", False),
                    damping_threshold=kn.get("damping_threshold", 0.3),
                    damping_strength=kn.get("damping_strength", 1.0))
    st = cases.make_state(cfg)
    sd = m.state_dict()
    for k, v in st.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v.copy())
    if case["learnable"]:
        # (the grid is bit-identical with the reference's; torch.log of the bandwidths may differ by an ulp between
        #  hosts, so the reference's initial knot tensors are part of the golden)
        assert np.array_equal(sd["spatial_basis.centers"].numpy(), g["in_centers"])
        sd["spatial_basis.centers"] = torch.from_numpy(g["in_centers"].copy())
        sd["spatial_basis.log_bandwidths"] = torch.from_numpy(g["in_log_bw"].copy())
    m.load_state_dict(sd)
    return m.to(dev())


def _dataset(arrays, p):
    from stnf.dataio.device_dataset import DeviceDataset
    X, coords, t, y = (torch.from_numpy(a).to(dev()) for a in arrays)
    return DeviceDataset(coords, t, y, X if p > 0 else None)


@pytest.mark.parametrize("name", list(tc.TRAIN_CASES))
def test_train_model_history_matches_the_reference(name, tmp_path):
    from stnf import training as T
    case = tc.TRAIN_CASES[name]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    achieved = json.load(open(os.path.join(GOLD, "training_achieved.json")))["cases"][name]
    cfg = tc.model_cfg(case)
    tr, va = tc.data(case, tc.TRAIN_ROWS, tc.VAL_ROWS)
    train, val = _dataset(tr, cfg["p"]), _dataset(va, cfg["p"])
    config = dict(case["config"], val_batch_size=tc.BATCH, verbose=False)
    m = _model(case, g)
    eng = T.make_engine(m, config, tc.BATCH, math.ceil(tc.TRAIN_ROWS / tc.BATCH))
    rates = []
    step = eng.step_indexed

    def stepping(*a, **kw):
        rates.append([eng.lr] + ([eng.basis_lr] if case["learnable"] else []))
        return step(*a, **kw)
    eng.step_indexed = stepping
    model, hist, _ = T.train_model(m, train, val, config, output_dir=tmp_path, shuffle=False, engine=eng)

    failures = []
    for col in ("train_loss", "val_loss", "val_rmse"):
        for e, (got, want) in enumerate(zip(hist[col], g["h64/" + col])):
            bound = max(4.0 * achieved[col][e], 1e-5 * abs(want))
            dist = abs(got - want)
            print(f"{name} {col}[{e}]: engine {got:.9g} float64 {want:.9g} |d| {dist:.3g} reference-f32 gap "
                  f"{achieved[col][e]:.3g} bound {bound:.3g} ratio {dist / bound:.3f}")
            if not dist <= bound:
                failures.append((col, e, got, float(want), dist, bound))
    assert len(hist["lr"]) == len(g["h64/lr"]) == case["config"]["epochs"]
    assert np.all(np.abs(np.asarray(hist["lr"]) - g["h64/lr"]) <= 1e-12 * g["h64/lr"])
    got_rates = np.asarray(rates, np.float64)
    assert got_rates.shape == g["rates"].shape
    assert np.all(np.abs(got_rates - g["rates"]) <= 1e-12 * np.abs(g["rates"]))
    assert not failures, failures
    # the model holds the best EMA state: the device-side copy, bit for bit, and so does model_best.pt
    assert eng.best_ema is not None and torch.equal(eng.flat, eng.best_ema)
    sd = torch.load(os.path.join(tmp_path, "model_best.pt"))
    for k, v in model.state_dict().items():
        assert torch.equal(sd[k], v.cpu()), k
