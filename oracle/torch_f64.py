"""float64 restatement of `stdadk_oracle.train_step_grads` in plain torch, for batches the dense numpy oracle cannot
hold (65 536 C2 rows would need a 5.4 GB feature matrix on the host).  TEST INFRASTRUCTURE ONLY.

Same arithmetic definition as the numpy oracle -- direct-difference distances (not the matmul expansion of cdist),
Wendland / Gaussian / triangular basis, Linear -> LayerNorm (biased variance) -> ReLU, MSE over B*Q -- evaluated in
float64 on any torch device, in row chunks: every row's forward and backward is row-local once the MSE scale
1/(B*Q) is passed in, so the gradients are float64 sums of per-chunk contributions.  Pinned against the numpy
oracle in tests/test_torch_f64_oracle.py.  `forward` is the forward half alone (the validation passes).
"""
import numpy as np
import torch

from . import stdadk_oracle as orc

F64 = torch.float64


def _t(a, device):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=device)


def _features(X, coords, t, cfg, knots, device):
    """[X(p) | phi level0.. | psi level0..] of one chunk in float64 (stdadk_oracle.model_forward)."""
    centers, bw, tc, tb = knots
    basis = cfg.get("basis", "wendland")
    c = _t(coords, device)
    dx = c[:, 0:1] - centers[None, :, 0]
    dy = c[:, 1:2] - centers[None, :, 1]
    r = torch.sqrt(dx * dx + dy * dy) / (bw[None, :] * orc.CALIBRATION_FACTORS[basis])
    if basis == "wendland":
        r = torch.clamp(r, max=1.0)
        phi = (1 - r) ** 6 * (35 * r * r + 18 * r + 3) / 3
    elif basis == "gaussian":
        phi = torch.exp(-0.5 * r * r)
    else:
        phi = torch.clamp(1 - r, min=0.0)
    s = (_t(t, device).reshape(-1, 1) - tc[None, :]) / tb[None, :]
    psi = torch.exp(-0.5 * s * s)
    if X is not None and np.asarray(X).size > 0 and cfg["p"] > 0:
        return torch.cat([_t(X, device), phi, psi], dim=1)
    return torch.cat([phi, psi], dim=1)


def _forward(a, layers, head, layernorm, masks=None):
    """`masks`: per hidden layer the keep-mask of these rows already scaled by 1 / (1 - p), or None."""
    cache = []
    for li, (W, b, g, be) in enumerate(layers):
        z = a @ W.T + b
        if layernorm:
            mu = z.mean(-1, keepdim=True)
            var = ((z - mu) ** 2).mean(-1, keepdim=True)
            rstd = 1.0 / torch.sqrt(var + orc.LN_EPS)
            xhat = (z - mu) * rstd
            u = xhat * g + be
        else:
            xhat, rstd, u = None, None, z
        cache.append((a, xhat, rstd, u))
        a = torch.clamp(u, min=0.0)
        if masks is not None:
            a = a * masks[li]
    Wo, bo = head
    return a @ Wo.T + bo, cache, a


def forward(X, coords, t, params, cfg, device="cpu", chunk=4096):
    """y_pred (B, Q) as `stdadk_oracle.model_forward(...)[0]` in eval mode, as numpy float64: the forward half of
    train_step_grads alone, for the validation passes (nothing is kept for a backward, any output width)."""
    device = torch.device(device)
    B = np.asarray(coords).shape[0]
    nh, ln = len(cfg["hidden_dims"]), cfg["layernorm"]
    layers_np, head_np, _ = orc.split_params(params, nh, ln)
    layers = [tuple(None if a is None else _t(a, device) for a in lay) for lay in layers_np]
    head = tuple(_t(a, device) for a in head_np)
    centers, bw, _ = orc.uniform_knots(cfg["k_spatial_centers"])
    tc, tb = orc.temporal_knots(cfg["k_temporal_centers"])
    knots = tuple(_t(a, device) for a in (centers, bw, tc, tb))
    ys = []
    for r0 in range(0, B, chunk):
        r1 = min(B, r0 + chunk)
        Xc = None if X is None else np.asarray(X)[r0:r1]
        a0 = _features(Xc, np.asarray(coords)[r0:r1], np.asarray(t)[r0:r1], cfg, knots, device)
        ys.append(_forward(a0, layers, head, ln)[0].cpu())
    return torch.cat(ys).numpy() if ys else np.zeros((0, head_np[0].shape[0]))


def train_step_grads(X, coords, t, y, params, cfg, device="cpu", chunk=4096, kink_tol=None, drop_masks=None,
                     drop_p=0.0):
    """(y_pred, loss, grads[, alts]) as `stdadk_oracle.train_step_grads`, as numpy float64.  `alts` (with kink_tol):
    the units within kink_tol of a ReLU kink in THIS forward, each with the change of every gradient when its ReLU
    derivative is taken from the other side -- taken from the numpy oracle on that single row (row-local), so
    `stdadk_oracle.fit_kink_sides` applies unchanged.  `drop_masks` / `drop_p` as `stdadk_oracle.mlp_forward`: keep-masks
    (B, h_l) per hidden layer, sliced per row chunk."""
    device = torch.device(device)
    dropping = drop_masks is not None and drop_p > 0
    B = np.asarray(coords).shape[0]
    nh, ln = len(cfg["hidden_dims"]), cfg["layernorm"]
    layers_np, head_np, keys = orc.split_params(params, nh, ln)
    layers = [tuple(None if a is None else _t(a, device) for a in lay) for lay in layers_np]
    head = tuple(_t(a, device) for a in head_np)
    centers, bw, _ = orc.uniform_knots(cfg["k_spatial_centers"])
    tc, tb = orc.temporal_knots(cfg["k_temporal_centers"])
    knots = tuple(_t(a, device) for a in (centers, bw, tc, tb))
    Q = np.asarray(y).reshape(B, -1).shape[1]
    scale = 1.0 / (B * Q)
    grads = {k: torch.zeros(np.asarray(params[k]).shape, dtype=F64, device=device) for k in params}
    loss = torch.zeros((), dtype=F64, device=device)
    ys, near = [], []
    for r0 in range(0, B, chunk):
        r1 = min(B, r0 + chunk)
        Xc = None if X is None else np.asarray(X)[r0:r1]
        a0 = _features(Xc, np.asarray(coords)[r0:r1], np.asarray(t)[r0:r1], cfg, knots, device)
        mk = [_t(m[r0:r1], device) / (1.0 - drop_p) for m in drop_masks] if dropping else None
        yp, cache, a_last = _forward(a0, layers, head, ln, mk)
        d = yp - _t(np.asarray(y)[r0:r1], device).reshape(yp.shape)
        loss += (d * d).sum()
        ys.append(yp.cpu())
        dy = 2.0 * d * scale
        ki = len(keys) - 1
        grads[f"mlp.{keys[ki]}.weight"] += dy.T @ a_last
        grads[f"mlp.{keys[ki]}.bias"] += dy.sum(0)
        da = dy @ head[0]
        ki -= 1
        for li in range(nh - 1, -1, -1):
            W, b, g, be = layers[li]
            a_in, xhat, rstd, u = cache[li]
            if mk is not None:
                da = da * mk[li]
            if kink_tol is not None:
                rr, cc = torch.nonzero(u.abs() < kink_tol, as_tuple=True)
                near += [(li, r0 + int(i), int(j)) for i, j in zip(rr.tolist(), cc.tolist())]
            du = da * (u > 0)
            if ln:
                grads[f"mlp.{keys[ki]}.weight"] += (du * xhat).sum(0)
                grads[f"mlp.{keys[ki]}.bias"] += du.sum(0)
                ki -= 1
                dxh = du * g
                dz = rstd * (dxh - dxh.mean(-1, keepdim=True) - xhat * (dxh * xhat).mean(-1, keepdim=True))
            else:
                dz = du
            grads[f"mlp.{keys[ki]}.weight"] += dz.T @ a_in
            grads[f"mlp.{keys[ki]}.bias"] += dz.sum(0)
            ki -= 1
            if li > 0:
                da = dz @ W
    y_pred = torch.cat(ys).numpy()
    out = (y_pred, float(loss) * scale, {k: v.cpu().numpy() for k, v in grads.items()})
    if kink_tol is None:
        return out
    alts = []
    for (li, r, c) in sorted(near):
        Xr = None if X is None else np.asarray(X)[r:r + 1]
        mr = [np.asarray(m)[r:r + 1] for m in drop_masks] if dropping else None
        yr, cache_r, _, _, _ = orc.model_forward(Xr, np.asarray(coords)[r:r + 1], np.asarray(t)[r:r + 1], params, cfg,
                                                 drop_masks=mr, drop_p=drop_p)
        yt = np.asarray(y)[r:r + 1]
        g0 = orc.mlp_mse_backward(yr, yt, cache_r, params, nh, ln, grad_scale=scale)
        g1 = orc.mlp_mse_backward(yr, yt, cache_r, params, nh, ln, grad_scale=scale, flip=((li, 0, c),))
        alts.append(((li, r, c), {k: g1[k] - g0[k] for k in g0}))
    return out + (alts,)
