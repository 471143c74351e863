"""GPU tests of the validation layer: stdadk_eval_indexed_f32 through stnf.evaluation.Evaluator against float64
(the oracle's predictions, numpy metrics), determinism and side effects, EMA weights without a swap, and the epoch
driver stnf.training.train_model end to end.  Bound against float64: the project's 1e-5 relative (test_gpu_parity)."""
import math
import os

import numpy as np
import pytest
import torch

from golden import cases
from oracle import stdadk_oracle as orc
from test_gpu_parity import build_learn_model, build_model, build_quantile_model, dev

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROWS, BATCH = 1000, 300          # 300 + 300 + 300 + 100: ragged last batch, no size a multiple of a 16/64-row tile


def _dataset(cfg, rows=ROWS):
    from stnf.dataio.device_dataset import DeviceDataset
    X, coords, t, y = cases.make_inputs(dict(cfg, B=rows))
    d = dev()
    ds = DeviceDataset(torch.from_numpy(coords).to(d), torch.from_numpy(t).to(d), torch.from_numpy(y).to(d),
                       torch.from_numpy(X).to(d) if cfg["p"] > 0 else None)
    return ds, (X, coords, t, y)


def _expected(yp, y, batch, taus=None, nc_weight=0.0, nc_power=1, extra=0.0):
    """Every key of Evaluator.evaluate in numpy float64 from float64 predictions yp (N,Q), targets y (N,1)."""
    yp, y = np.asarray(yp, np.float64), np.asarray(y, np.float64).reshape(-1, 1)
    n, Q = yp.shape
    col = yp[:, Q // 2:Q // 2 + 1]
    out = {"mse": np.mean((col - y) ** 2), "mae": np.mean(np.abs(col - y))}
    out["rmse"] = math.sqrt(out["mse"])
    per_batch = []
    for s in range(0, n, batch):
        pb, yb = yp[s:s + batch], y[s:s + batch]
        if taus is None:
            per_batch.append(np.mean((pb - yb) ** 2))
        else:
            e = yb - pb
            tq = np.asarray(taus, np.float64)[None, :]
            obj = np.mean(np.maximum((tq - 1) * e, tq * e))
            if nc_weight > 0 and Q > 1:
                d = np.maximum(pb[:, :-1] - pb[:, 1:], 0.0)
                obj += nc_weight * np.mean(np.sum(d if nc_power == 1 else d * d, axis=1))
            per_batch.append(obj + extra)
    out["loss"] = float(np.mean(per_batch))
    if taus is not None:
        e = y - yp
        tq = np.asarray(taus, np.float64)[None, :]
        checks = np.mean(np.maximum((tq - 1) * e, tq * e), axis=0)
        if Q == 1:
            out["check_loss"] = float(checks[0])
        else:
            out["mean_check_loss"] = out["check_loss"] = float(np.mean(checks))
            out["crps"] = float(orc.crps(yp, y[:, 0], list(taus)))
    return out


def _compare(got, want, what):
    assert got["rows"] == ROWS
    for k, w in want.items():
        print(f"{what}: {k} got {got[k]:.12g} float64 {w:.12g} rel {abs(got[k] - w) / max(abs(w), 1e-300):.3g}")
    for k, w in want.items():
        assert abs(got[k] - w) <= TOL * abs(w), (what, k, got[k], w)
    assert set(want) <= set(got)


@pytest.mark.parametrize("name,dense", [("tiny9_ln_p3", False), ("default227", False), ("default227", True),
                                        ("default227_gauss", False), ("default227_tri", False)])
def test_metrics_match_float64_mse(name, dense):
    from stnf.evaluation import Evaluator
    cfg = cases.MODEL_CASES[name]
    m = build_model(cfg).eval()
    ds, (X, coords, t, y) = _dataset(cfg)
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    yp = orc.model_forward(X, coords, t, params, cfg)[0]
    got = Evaluator(m, max_batch=BATCH, force_dense=dense).evaluate(ds, BATCH)
    _compare(got, _expected(yp, y, BATCH), f"{name} dense={dense}")


@pytest.mark.parametrize("name", ["tiny9_q90", "tiny9_mq5_nc1", "tiny9_mq5_nc2", "tiny9_delta5", "default227_q10",
                                  "default227_mq5", "default227_delta5"])
@pytest.mark.parametrize("dense", [False, True])
def test_metrics_match_float64_quantile(name, dense):
    from stnf.evaluation import Evaluator
    m, cfg, lc = build_quantile_model(name)
    m.eval()
    ds, (X, coords, t, y) = _dataset(cfg)
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    extra = 0.0
    if lc.get("delta"):
        std, delta, _ = orc.delta_to_standard(params, cfg)
        if lc.get("nc_lambda", 0.0) > 0:
            extra = lc["nc_lambda"] * orc.p_nc_delta(delta)[0]
    else:
        std = params
    yp = orc.model_forward(X, coords, t, std, cfg)[0]
    ev = Evaluator(m, loss="pinball", quantile_levels=lc["taus"], non_crossing_weight=lc.get("nc_weight", 0.0),
                   non_crossing_power=lc.get("nc_power", 1), non_crossing_lambda=lc.get("nc_lambda", 0.0),
                   max_batch=BATCH, force_dense=dense)
    got = ev.evaluate(ds, BATCH)
    want = _expected(yp, y, BATCH, lc["taus"], 0.0 if lc.get("delta") else lc.get("nc_weight", 0.0),
                     lc.get("nc_power", 1), extra)
    _compare(got, want, f"{name} dense={dense}")


@pytest.mark.parametrize("dense", [False, True])
def test_metrics_match_float64_learnable(dense):
    from stnf.evaluation import Evaluator
    m, cfg, kn, g = build_learn_model("default227_learn")
    m.eval()
    ds, (X, coords, t, y) = _dataset(cfg)
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    tc, tb = orc.temporal_knots(cfg["k_temporal_centers"])
    phi = orc.spatial_basis(coords, g["in_centers"].astype(np.float64), np.exp(g["in_log_bw"].astype(np.float64)),
                            cfg["basis"])
    feat = orc.features(X, phi, orc.temporal_basis(t, tc, tb), cfg["p"])
    yp = orc.mlp_forward(feat, params, len(cfg["hidden_dims"]), cfg["layernorm"])[0]
    got = Evaluator(m, max_batch=BATCH, force_dense=dense).evaluate(ds, BATCH)
    _compare(got, _expected(yp, y, BATCH), f"default227_learn dense={dense}")


def _engine(cfg, build=build_model, **kw):
    from stnf.engine import TrainStep
    m = build(cfg) if build is build_model else build
    o = cases.OPT
    return TrainStep(m.train(), lr=o["lr"], weight_decay=o["weight_decay"], grad_clip=o["grad_clip"],
                     ema_decay=o["ema_decay"], max_batch=BATCH, seed=3, **kw)


def _state(eng):
    return [x.clone() for x in (eng.flat, eng.m, eng.v, eng.ema, eng.step_dev)]


def _steps(eng, ds, n, start=0):
    for i in range(start, start + n):
        idx = torch.arange(i * 100, i * 100 + BATCH, device=ds.coords.device) % ROWS
        eng.step_indexed(ds.coords, ds.t, ds.y, idx, X_all=ds.X)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_determinism_and_no_side_effects(dtype):
    from stnf.evaluation import Evaluator
    cfg = cases.MODEL_CASES["default227"]
    ds, _ = _dataset(cfg)
    a, b = _engine(cfg, dtype=dtype), _engine(cfg, dtype=dtype)
    _steps(a, ds, 2)
    _steps(b, ds, 2)
    before = _state(a)
    ev = Evaluator(a.model, max_batch=BATCH)
    r1 = ev.evaluate(ds, BATCH, params="ema", engine=a)
    s1 = list(ev.sums)
    r2 = ev.evaluate(ds, BATCH, params="ema", engine=a)
    assert s1 == ev.sums and r1 == r2, "two evaluations of the same data differ"
    live1 = ev.evaluate(ds, BATCH, params="live", engine=a)
    s_live = list(ev.sums)
    ev.evaluate(ds, BATCH, params="live", engine=a)
    assert s_live == ev.sums
    assert live1["loss"] != r1["loss"]                      # (the shadow lags the live weights)
    for x, y in zip(before, _state(a)):
        assert torch.equal(x, y), "evaluate() changed the engine's state"
    _steps(a, ds, 1, start=2)
    _steps(b, ds, 1, start=2)
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y), "a step after evaluate() differs from the step without it"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ema_views_equal_ema_swap(dtype):
    from stnf.evaluation import Evaluator
    cfg = cases.MODEL_CASES["default227"]
    ds, _ = _dataset(cfg)
    eng = _engine(cfg, dtype=dtype)
    _steps(eng, ds, 3)
    ev = Evaluator(eng.model, max_batch=BATCH)
    assert Evaluator.ema_in_place(eng)
    ev.evaluate(ds, BATCH, params="ema", engine=eng)
    in_place = list(ev.sums)
    eng.swap_in_ema()
    ev.evaluate(ds, BATCH, params="live", engine=eng)
    swapped = list(ev.sums)
    eng.swap_in_ema()
    print("in place", in_place[:5], "swapped", swapped[:5])
    assert in_place == swapped


def test_ema_through_swap_for_learnable_knots_leaves_state():
    from stnf.evaluation import Evaluator
    m, cfg, kn, g = build_learn_model("default227_learn")
    ds, _ = _dataset(cfg)
    eng = _engine(cfg, build=m)
    _steps(eng, ds, 2)
    before = _state(eng)
    ev = Evaluator(m, max_batch=BATCH)
    assert not Evaluator.ema_in_place(eng)
    r = ev.evaluate(ds, BATCH, params="ema", engine=eng)
    assert math.isfinite(r["loss"]) and r["rows"] == ROWS
    for x, y in zip(before, _state(eng)):
        assert torch.equal(x, y)


def test_train_model_end_to_end(tmp_path):
    """3 epochs, warm-up 1, ragged last batch: train_loss is the mean of batch means (checked against per-batch reads of
    a second engine), the returned model holds the best EMA state bitwise, and evaluating it reproduces that epoch's
    validation numbers exactly (deterministic metrics)."""
    from stnf import training as T
    cfg = cases.MODEL_CASES["default227"]
    tr, _ = _dataset(cfg)
    va, _ = _dataset(dict(cfg, seed=99), rows=700)
    config = {"lr": 2e-2, "epochs": 3, "batch_size": BATCH, "warmup_epochs": 1, "scheduler": "cosine", "grad_clip": 10.0,
              "patience": 5, "verbose": False, "dropout_seed": 5}
    m = build_model(cfg)
    eng = T.make_engine(m, config, BATCH, math.ceil(ROWS / BATCH))
    model, hist, _ = T.train_model(m, tr, va, config, output_dir=tmp_path, shuffle=False, engine=eng)
    print("history", hist)
    assert all(math.isfinite(v) for k in hist for v in hist[k]) and len(hist["val_loss"]) == 3
    best = int(np.argmin(hist["val_loss"]))
    assert torch.equal(eng.flat, eng.best_ema)
    again = T.evaluate_model(model, va, dict(config, val_batch_size=T.val_batch_size(BATCH, len(va))))
    assert again["loss"] == hist["val_loss"][best] and again["rmse"] == hist["val_rmse"][best]
    sd = torch.load(os.path.join(tmp_path, "model_best.pt"))
    for k, v in model.state_dict().items():
        assert torch.equal(sd[k], v.cpu()), k
    # the first epoch again, reading the accumulator after every batch
    m2 = build_model(cfg)
    e2 = T.make_engine(m2, config, BATCH, math.ceil(ROWS / BATCH))
    nb = math.ceil(ROWS / BATCH)
    means = []
    for i, idx in enumerate(tr.epoch_batches(BATCH, shuffle=False)):
        e2.set_lr(2e-2 if i == 0 else 2e-2 * i / nb)
        e2.step_indexed(tr.coords, tr.t, tr.y, idx, X_all=tr.X)
        means.append(e2.mean_loss())
    want = float(np.mean(means))
    print("train_loss", hist["train_loss"][0], "per-batch reads", want)
    assert abs(hist["train_loss"][0] - want) <= 1e-6 * want       # (float atomics of the training accumulator)


@pytest.mark.parametrize("check_every", [0, 1])
def test_train_model_nan_batch(check_every):
    """A NaN target in the second batch (scripts/train_st_interp.py:724-733): NaN train_loss, a validation loss that
    never becomes best, the final EMA state loaded -- whether the epoch runs through (default) or is left at the
    batch (`nan_check_every`)."""
    from stnf import training as T
    cfg = cases.MODEL_CASES["default227"]
    tr, _ = _dataset(cfg)
    va, _ = _dataset(dict(cfg, seed=99), rows=700)
    tr.y[BATCH + 5, 0] = float("nan")
    config = {"lr": 2e-2, "epochs": 2, "batch_size": BATCH, "grad_clip": 10.0, "patience": 5, "verbose": False,
              "nan_check_every": check_every}
    m = build_model(cfg)
    eng = T.make_engine(m, config, BATCH, math.ceil(ROWS / BATCH))
    _, hist, _ = T.train_model(m, tr, va, config, shuffle=False, engine=eng)
    assert all(math.isnan(v) for v in hist["train_loss"]) and all(math.isnan(v) for v in hist["val_loss"])
    assert eng.best_ema is None and eng.first_nonfinite_step() == 2
    assert (eng.stopped_at is not None) == bool(check_every)
    assert torch.equal(eng.flat.view(torch.int32), eng.ema.view(torch.int32))      # (NaNs: compare the bits)
