"""The chunked float64 torch restatement of the oracle (oracle/torch_f64.py), which the large-batch GPU tests use
as their reference, against the numpy oracle itself: y, loss, every gradient and the near-kink alternatives."""
import numpy as np
import pytest

from golden import cases
from oracle import stdadk_oracle as orc
from oracle import torch_f64


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("name,chunk", [("tiny9", 3), ("default227", 64), ("default227", 4096),
                                        ("default227_tri", 16), ("c2_b257", 100)])
def test_chunked_float64_step_equals_numpy_oracle(name, chunk):
    cfg = cases.MODEL_CASES[name]
    X, coords, t, y = cases.make_inputs(cfg)
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    yo, lo, go = orc.train_step_grads(X, coords, t, y, params, cfg)
    yt, lt, gt = torch_f64.train_step_grads(X, coords, t, y, params, cfg, device="cpu", chunk=chunk)
    assert cfg["B"] % chunk != 0 or chunk >= cfg["B"] or name == "tiny9"
    assert yt.shape == yo.shape and _rel(yt, yo) <= 1e-12
    assert abs(lt - lo) <= 1e-12 * lo
    assert set(gt) == set(go)
    for k in go:
        assert gt[k].shape == go[k].shape, k
        assert _rel(gt[k], go[k]) <= 1e-12, (k, _rel(gt[k], go[k]))
    # the knots no row reaches: exactly zero dW0 columns in both
    z = np.abs(go["mlp.0.weight"]).sum(0) == 0
    assert np.array_equal(np.abs(gt["mlp.0.weight"]).sum(0) == 0, z)


@pytest.mark.parametrize("name,chunk", [("tiny9", 3), ("tiny9_ln_p3", 4), ("default227", 64), ("default227_tri", 16),
                                        ("c2_b257", 100), ("tiny9_mq5_nc2", 2), ("c2_b257_mq3", 4096)])
def test_chunked_float64_forward_equals_numpy_oracle(name, chunk):
    """The forward-only entry point (the reference of the production validation calls), quantile heads included."""
    cfg = cases.MODEL_CASES[name] if name in cases.MODEL_CASES else cases.quantile_cfg(name)[0]
    X, coords, t, _ = cases.make_inputs(cfg)
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    yo = orc.model_forward(X, coords, t, params, cfg)[0]
    yt = torch_f64.forward(X, coords, t, params, cfg, device="cpu", chunk=chunk)
    assert yt.shape == yo.shape == (cfg["B"], cfg["output_dim"]) and yt.dtype == np.float64
    assert _rel(yt, yo) <= 1e-12, _rel(yt, yo)
    assert np.abs(yt - yo).max() <= 1e-12 * max(1.0, np.abs(yo).max())


def test_chunked_float64_near_kink_units_equal_numpy_oracle():
    """With a kink tolerance wide enough to catch units, the restatement lists the same units, with the same
    per-unit gradient changes, as the numpy oracle (chunk boundaries falling inside the batch)."""
    cfg = cases.MODEL_CASES["default227"]
    X, coords, t, y = cases.make_inputs(cfg)
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    tol = 1e-2
    *_, ao = orc.train_step_grads(X, coords, t, y, params, cfg, kink_tol=tol)
    *_, at = torch_f64.train_step_grads(X, coords, t, y, params, cfg, device="cpu", chunk=50, kink_tol=tol)
    assert len(ao) > 0
    assert [u for u, _ in at] == sorted(u for u, _ in ao)
    do = dict(ao)
    for u, d in at:
        for k in d:
            # (a single-row forward rounds its matmuls differently from the whole batch's, ~1e-16 relative, and a
            # unit's change is a difference of two near-equal backward passes: ~1e-12 relative, checked at 1e-10)
            assert _rel(d[k], do[u][k]) <= 1e-10, (u, k)
