#!/usr/bin/env python3
"""Goldens of the DA-STDK row of the reference's Table 4.4: learnable knots + delta head + P_nc(delta), by importing the
REAL reference (as make_golden.py does; build container only).

    python tests/golden/make_delta_learn_golden.py      # rewrites the two .npz files and delta_learn_achieved.json

Cases: delta_learn_cases.DELTA_LEARN_CASES.  Same keys as the other goldens: y64, loss64, the g / p / ema digests,
opt_losses64, the reference's float32 results beside them, plus the case's fp32 knot inputs and the pieces of the
objective in float64 (check64, pnc64, domain_pen64, movement_pen64).  The batch body is the driver's
(scripts/train_st_interp.py:617-712): check loss per level + nc_lambda * P_nc(delta) + knot penalties, damping hook,
per-group clipping, two-group AdamW, EMA.

Asserted in float64 at the state of every one of OPT['steps'] steps, so that the reference alone stays clear of
sub-gradient ties: |delta_k0 - S_k| > TIE_MARGIN for every k >= 1, both signs of S_k - delta_k0 occur, and no check-loss
residual is exactly zero.  Both signs of the residual in every output column are asserted at the start state (the
single-gradient golden and step 1).  At steps 2 and 3 they CANNOT hold on these bases: OPT's learning rate of 2e-2
moves every parameter by about lr in the first AdamW step and swings whole output columns past every target.  Where
that happens is recorded as data, not hidden: `resid_pos64` / `resid_neg64` [steps, Q] hold the counts of positive and
negative residuals per step and column, and `resid_minabs64` [steps] the smallest |residual| (the distance from the
check loss's own kink), so a reader sees which (step, column) pairs are one-signed and that none sits on a tie.

delta_learn_achieved.json: per tensor, the reference's own float32-against-float64 deviation in the norm
test_gpu_parity.check_vs_digest uses (relative l2), and the largest loss deviation over the steps."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference on the path)
import scripts.train_st_interp as ref_train  # noqa: E402
from golden import cases  # noqa: E402
from golden import delta_learn_cases as dl  # noqa: E402

mg.ref_train = ref_train


def build(cfg, kn):
    """make_golden.build_learn with the delta head and this file's start state."""
    model = mg.STInterpMLP(p=cfg["p"], k_spatial_centers=cfg["k_spatial_centers"],
                           k_temporal_centers=cfg["k_temporal_centers"], hidden_dims=cfg["hidden_dims"], dropout=0.0,
                           layernorm=cfg["layernorm"], spatial_learnable=True, spatial_init_method="uniform",
                           spatial_basis_function=cfg["basis"], output_dim=cfg["output_dim"],
                           use_delta_reparameterization=True,
                           gradient_damping=kn.get("gradient_damping", False),
                           damping_threshold=kn.get("damping_threshold", 0.3),
                           damping_strength=kn.get("damping_strength", 1.0))
    sb = model.spatial_basis
    dc, dlb = cases.knot_perturbation(cfg)
    c0 = (sb.centers.detach().numpy() + dc).astype(np.float32)
    lb0 = (sb.log_bandwidths.detach().numpy() + dlb).astype(np.float32)
    st = dl.make_state(cfg)
    sd = model.state_dict()
    for k, v in st.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v.copy())
    sd["spatial_basis.centers"] = torch.from_numpy(c0.copy())
    sd["spatial_basis.log_bandwidths"] = torch.from_numpy(lb0.copy())
    model.load_state_dict(sd)
    return model, c0, lb0


def loss_of(model, X, coords, t, y, kn, lc, yp=None):
    yp = model(X, coords, t) if yp is None else yp
    loss = mg.n3_loss(model, yp, y, lc)
    if kn.get("domain_penalty_weight", 0.0) > 0:
        loss = loss + kn["domain_penalty_weight"] * model.compute_domain_penalty()
    if kn.get("movement_penalty_weight", 0.0) > 0:
        loss = loss + kn["movement_penalty_weight"] * model.compute_movement_penalty()
    return loss


def clear_of_ties(model, yp, y, where, both_signs=True, log=None):
    """The conditions of the module docstring on the model's present state (float64 runs only).  `log`: a list that
    receives (positives per column, negatives per column, smallest |residual|)."""
    if yp.dtype != torch.float64:
        return
    ds = [p.detach() for p in model.get_delta_parameters()]
    diff = np.array([float(torch.clamp(-dk[1:], min=0.0).sum() - dk[0]) for dk in ds[1:]])
    assert (np.abs(diff) > dl.TIE_MARGIN).all(), (where, diff)
    assert (diff > 0).any() and (diff < 0).any(), (where, diff)
    e = (y - yp.detach()).numpy()
    if both_signs:
        assert ((e > 0).any(0) & (e < 0).any(0)).all(), (where, (e > 0).sum(0), (e < 0).sum(0))
    assert (e != 0).all(), where
    if log is not None:
        log.append(((e > 0).sum(0), (e < 0).sum(0), np.abs(e).min(), diff))
    return diff


def run(model, X, coords, t, y, kn, lc):
    model.train()
    model.zero_grad()
    yp = model(X, coords, t)
    clear_of_ties(model, yp, y, "gradient")
    loss = loss_of(model, X, coords, t, y, kn, lc, yp)
    loss.backward()
    return yp.detach(), loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def opt(model, X, coords, t, y, kn, lc, log=None):
    """make_golden.learn_opt's two-group loop on this objective."""
    o = cases.OPT
    basis_params = list(model.spatial_basis.parameters())
    mlp_params = [p for p in model.parameters() if not any(p is bp for bp in basis_params)]
    optim = torch.optim.AdamW([{"params": mlp_params, "lr": o["lr"]},
                               {"params": basis_params, "lr": o["lr"] * cases.BASIS_LR_RATIO}],
                              weight_decay=o["weight_decay"], betas=o["betas"], eps=o["eps"])
    ema = mg.ModelEMA(model, decay=o["ema_decay"])
    losses = []
    model.train()
    for s in range(o["steps"]):
        optim.zero_grad()
        yp = model(X, coords, t)
        clear_of_ties(model, yp, y, f"step {s + 1}", both_signs=(s == 0), log=log)
        loss = loss_of(model, X, coords, t, y, kn, lc, yp)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(basis_params, o["grad_clip"] * cases.BASIS_CLIP_RATIO)
        torch.nn.utils.clip_grad_norm_(mlp_params, o["grad_clip"])
        optim.step()
        ema.update(model)
        losses.append(float(loss.detach()))
    return ({n: p.detach().clone() for n, p in model.named_parameters()},
            {n: v.detach().clone() for n, v in ema.shadow.items()}, np.array(losses, dtype=np.float64))


def gen(name):
    cfg, kn, lc = dl.cfg_of(name)
    X, coords, t, y = (torch.from_numpy(a) for a in cases.make_inputs(cfg))
    d = (X.double(), coords.double(), t.double(), y.double())
    out = {}
    m32, c0, lb0 = build(cfg, kn)
    out["in_centers"], out["in_log_bw"] = c0, lb0
    # (centers_init, the unperturbed grid, is not stored: it is cases' own grid, and the C2 file has to stay under the
    #  size limit of a committed file)
    y32, l32, g32 = run(m32, X, coords, t, y, kn, lc)
    m64 = build(cfg, kn)[0].double()
    y64, l64, g64 = run(m64, *d, kn, lc)
    out["y64"] = y64.numpy()
    out["yerr32_maxabs"] = np.float64(np.abs(y32.numpy().astype(np.float64) - y64.numpy()).max())
    out["loss32"], out["loss64"] = np.float32(l32.item()), np.float64(l64.item())
    out["check64"] = np.array([float(ref_train.quantile_loss(y64[:, i:i + 1], d[3], q)) for i, q in enumerate(lc["taus"])])
    out["pnc64"] = np.float64(ref_train.compute_p_nc_delta_penalty(m64.get_delta_parameters()).item())
    out["domain_pen64"] = np.float64(m64.compute_domain_penalty().item())
    out["movement_pen64"] = np.float64(m64.compute_movement_penalty().item())
    ach = {"g": {}, "p": {}, "ema": {}}
    for k in g64:
        mg.store(out, "g", k, g64[k].numpy(), g32[k].numpy(), cfg["seed"] + 7, False)
        ach["g"][k] = float(out[f"gerr32_rell2/{k}"])
    p32, s32, ls32 = opt(build(cfg, kn)[0], X, coords, t, y, kn, lc)
    log = []
    p64, s64, ls64 = opt(build(cfg, kn)[0].double(), *d, kn, lc, log)
    out["opt_losses32"], out["opt_losses64"] = ls32, ls64
    out["resid_pos64"] = np.stack([a for a, _, _, _ in log]).astype(np.int64)
    out["resid_neg64"] = np.stack([b for _, b, _, _ in log]).astype(np.int64)
    out["resid_minabs64"] = np.array([c for _, _, c, _ in log], dtype=np.float64)
    out["tie_diff64"] = np.stack([dd for _, _, _, dd in log])          # S_k - delta_k0, k = 1..Q-1, per step
    for k in p64:
        mg.store(out, "p", k, p64[k].numpy(), p32[k].numpy(), cfg["seed"] + 7, False)
        mg.store(out, "ema", k, s64[k].numpy(), s32[k].numpy(), cfg["seed"] + 7, False)
        ach["p"][k] = float(out[f"perr32_rell2/{k}"])
        ach["ema"][k] = float(out[f"emaerr32_rell2/{k}"])
    ach["losses_maxabs"] = float(np.abs(ls32 - ls64).max())
    ach["losses_scale"] = float(max(1.0, np.abs(ls64).max()))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.0f} KiB  loss64={out['loss64']:.6f} pnc64={out['pnc64']:.6f} "
          f"losses64={ls64} worst ref fp32 err p={max(ach['p'].values()):.2e} ema={max(ach['ema'].values()):.2e} "
          f"losses={ach['losses_maxabs']:.2e}")
    return ach


if __name__ == "__main__":
    torch.manual_seed(0)
    achieved = {name: gen(name) for name in dl.DELTA_LEARN_CASES}
    with open(os.path.join(HERE, dl.ACHIEVED), "w") as f:
        json.dump(achieved, f, indent=1, sort_keys=True)
        f.write("\n")
