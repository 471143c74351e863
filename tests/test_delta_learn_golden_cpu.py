"""Sanity of the DA-STDK goldens (learnable knots + delta head + P_nc(delta), tests/golden/make_delta_learn_golden.py)
on the CPU: the stored float64 objective is the sum of its parts as the oracle computes them from the stored
predictions and the case's start state, and that start state is clear of the sub-gradient ties the generator watches."""
import json
import os

import numpy as np
import pytest

from golden import cases
from golden import delta_learn_cases as dl
from oracle import stdadk_oracle as orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _delta(cfg):
    st = dl.make_state(cfg)
    return np.stack([st[f"delta_params.{k}"] for k in range(cfg["output_dim"])]).astype(np.float64)


@pytest.mark.parametrize("name", list(dl.DELTA_LEARN_CASES))
def test_loss64_is_the_sum_of_its_parts(name):
    cfg, kn, lc = dl.cfg_of(name)
    g = np.load(os.path.join(GOLD, name + ".npz"))
    _, _, _, y = cases.make_inputs(cfg)
    check = orc.quantile_objective(g["y64"], y, lc["taus"])[0]
    pnc = orc.p_nc_delta(_delta(cfg))[0]
    dom = orc.domain_penalty(g["in_centers"].astype(np.float64))[0]
    assert kn.get("movement_penalty_weight", 0.0) == 0.0          # (both bases: no movement penalty, nothing to add)
    want = check + lc["nc_lambda"] * pnc + kn.get("domain_penalty_weight", 0.0) * dom
    got = float(g["loss64"])
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert abs(pnc - float(g["pnc64"])) <= 1e-12 * abs(pnc) and abs(dom - float(g["domain_pen64"])) <= 1e-12 * max(dom, 1e-300)
    assert abs(np.mean(g["check64"]) - check) <= 1e-12 * abs(check)
    assert abs(got - float(g["opt_losses64"][0])) <= 1e-12 * abs(got)      # step 1 starts from the same state


@pytest.mark.parametrize("name", list(dl.DELTA_LEARN_CASES))
def test_start_state_is_clear_of_ties(name):
    cfg, kn, lc = dl.cfg_of(name)
    g = np.load(os.path.join(GOLD, name + ".npz"))
    d = _delta(cfg)
    diff = np.array([np.maximum(-d[k, 1:], 0.0).sum() - d[k, 0] for k in range(1, d.shape[0])])
    assert (np.abs(diff) > dl.TIE_MARGIN).all(), diff
    assert (diff > 0).any() and (diff < 0).any(), diff
    _, _, _, y = cases.make_inputs(cfg)
    e = y.astype(np.float64) - g["y64"]
    assert ((e > 0).any(0) & (e < 0).any(0)).all() and (e != 0).all()
    # what the generator recorded: the start state's row agrees, every step stays off the delta tie and off e == 0
    steps = cases.OPT["steps"]
    assert g["resid_pos64"].shape == g["resid_neg64"].shape == (steps, cfg["output_dim"])
    assert np.array_equal(g["resid_pos64"][0], (e > 0).sum(0)) and np.array_equal(g["resid_neg64"][0], (e < 0).sum(0))
    assert (g["resid_pos64"] + g["resid_neg64"] == cfg["B"]).all() and (g["resid_minabs64"] > 0).all()
    td = g["tie_diff64"]
    assert td.shape == (steps, cfg["output_dim"] - 1) and np.allclose(td[0], diff, rtol=0, atol=1e-12)
    assert (np.abs(td) > dl.TIE_MARGIN).all() and ((td > 0).any(1) & (td < 0).any(1)).all()


def test_achieved_file_names_every_tensor():
    with open(os.path.join(GOLD, dl.ACHIEVED)) as f:
        ach = json.load(f)
    assert sorted(ach) == sorted(dl.DELTA_LEARN_CASES)
    for name, a in ach.items():
        cfg, _, _ = dl.cfg_of(name)
        keys = ["spatial_basis.centers", "spatial_basis.log_bandwidths"] + list(dl.make_state(cfg))
        assert sorted(a["p"]) == sorted(a["ema"]) == sorted(a["g"]) == sorted(keys)
        assert all(v >= 0 for v in a["p"].values()) and a["losses_maxabs"] >= 0 and a["losses_scale"] >= 1
