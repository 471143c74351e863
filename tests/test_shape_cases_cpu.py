"""The float64 reference of the shape matrix (tests/golden/shape_cases.py) on its own, before any kernel is compared
with it: the numpy oracle and its chunked torch restatement (oracle/torch_f64.py, pinned so far at the shipped shapes
only) agree on y, loss and every gradient at every width, depth and head of the matrix, and the inputs keep clear of
the ReLU kinks (at most two hidden units within 1e-6 of one: a condition on the seeds, not on the kernels)."""
import numpy as np
import pytest

from golden import cases
from golden import shape_cases as SC
from oracle import stdadk_oracle as orc
from oracle import torch_f64

KINK_TOL = 1e-6


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_matrix_is_what_the_kernels_need():
    """The properties the cases are named after: feature widths of the d_* cases, first widths of the window cases,
    widths inside / outside what the fused tail takes."""
    for name, cfg in SC.SHAPE_CASES.items():
        D = cfg["p"] + sum(cfg["k_spatial_centers"]) + sum(cfg["k_temporal_centers"])
        tail = all(h % 16 == 0 and h <= 256 for h in cfg["hidden_dims"]) and 1 <= len(cfg["hidden_dims"]) <= 8 \
            and cfg["output_dim"] <= 8
        if name in SC.WINDOW_CASES:
            assert cfg["hidden_dims"][0] in (128, 256) and cfg["basis"] == "wendland" and tail and D == 569
        elif name in SC.DENSE0_CASES:
            assert D == SC.FEATURE_WIDTH[name] and cfg["hidden_dims"][0] not in (128, 256) and tail
        else:
            assert name in SC.FALLBACK_CASES and not tail
        assert cfg["B"] == 300
    seeds = [c["seed"] for c in SC.SHAPE_CASES.values()]
    assert len(set(seeds)) == len(seeds)
    assert {c["seed"] for c in cases.MODEL_CASES.values()}.isdisjoint(seeds)


@pytest.mark.parametrize("name", list(SC.SHAPE_CASES))
def test_float64_references_agree_and_inputs_avoid_kinks(name):
    cfg = SC.config(name)
    X, coords, t, y = SC.make_inputs(cfg)
    assert y.shape == (cfg["B"], cfg["output_dim"])
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    yo, lo, go, alts = orc.train_step_grads(X, coords, t, y, params, cfg, kink_tol=KINK_TOL)
    yt, lt, gt, at = torch_f64.train_step_grads(X, coords, t, y, params, cfg, device="cpu", chunk=128,
                                                kink_tol=KINK_TOL)
    assert yt.shape == yo.shape == y.shape and _rel(yt, yo) <= 1e-12
    assert abs(lt - lo) <= 1e-12 * lo
    assert set(gt) == set(go) == set(params)
    worst = 0.0
    for k in go:
        assert gt[k].shape == go[k].shape == params[k].shape, k
        assert np.linalg.norm(go[k]) > 0, k
        worst = max(worst, _rel(gt[k], go[k]))
        assert _rel(gt[k], go[k]) <= 1e-12, (k, _rel(gt[k], go[k]))
    print(f"{name}: loss {lo:.6f}, numpy vs torch float64 worst gradient rel-L2 {worst:.1e}, {len(alts)} units within "
          f"{KINK_TOL} of a kink")
    assert [u for u, _ in at] == sorted(u for u, _ in alts)
    assert len(alts) <= 2, [u for u, _ in alts]
