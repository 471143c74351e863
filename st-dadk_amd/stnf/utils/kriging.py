"""Local ordinary kriging on a neighbour table (stdadk_krige_weights_f64, stdadk_krige_apply_f32; include/stdadk.h).

Per row of a table of `baselines.knn_host` / stdadk_knn_f32 the ordinary-kriging system of its first k entries under ONE
variogram model gamma(h) = nugget + psill (1 - rho(h / range)) -- exponential, spherical or gaussian -- is solved by
Cholesky in the fixed order of the contract; the weights sum to 1 and the kriging variance, that of a new noisy
observation, turns the prediction into Gaussian quantiles `prediction + z_tau * sd`.  The nugget sits on the diagonal
only, so a target on top of a source does not reproduce it when nugget > 0: the prediction is of the smooth signal.

`kriging_weights_host` and `kriging_apply_host` are the two contracts in numpy float64, one rounded operation per
contract operation in the contract's order, vectorised over the rows only: the path of `device: cpu` and the tests'
restatement (bit for bit with the spherical model; exp's last bits differ between the libraries for the other two).
`device_kriging_weights` wraps the device call.  The model comes from `variogram.fit_variogram`.

Not built: universal and space-time kriging, anisotropy, a global (non-local) solve, covariates.
"""
from statistics import NormalDist

import numpy as np
import torch

MODELS = ("exponential", "spherical", "gaussian")      # STDADK_KRIGE_EXPONENTIAL, _SPHERICAL, _GAUSSIAN
MAX_K = 16                                      # STDADK_KNN_MAX_K
MAX_COLS = 8                                    # STDADK_KRIGE_MAX_COLS
_BLOCK_ROWS = 4096                              # rows per block of the host restatement ((rows, k, k) arrays)
_span = range                                   # (the contract's parameter `range` shadows the builtin below)


def model_code(model):
    """0 / 1 / 2 for a model's name, or the code itself."""
    if isinstance(model, str):
        if model not in MODELS:
            raise ValueError(f"kriging: model '{model}' must be one of {MODELS}")
        return MODELS.index(model)
    if int(model) not in (0, 1, 2):
        raise ValueError(f"kriging: model={model} outside 0..2")
    return int(model)


def check_params(nugget, psill, range_):
    nugget, psill, range_ = float(nugget), float(psill), float(range_)
    if not (np.isfinite([nugget, psill, range_]).all() and nugget >= 0.0 and psill >= 0.0 and nugget + psill > 0.0
            and np.isfinite(nugget + psill) and range_ > 0.0):
        raise ValueError(f"kriging: nugget={nugget} and psill={psill} must be finite, >= 0 and not both 0, "
                         f"range={range_} finite and > 0")
    return nugget, psill, range_


def normal_quantiles(levels):
    """The standard-normal quantile of every level in (0, 1), float64; exactly 0 for 0.5."""
    levels = [float(q) for q in levels]
    if any(not 0.0 < q < 1.0 for q in levels):
        raise ValueError(f"kriging: quantile levels must lie strictly between 0 and 1, got {levels}")
    return np.asarray([0.0 if q == 0.5 else NormalDist().inv_cdf(q) for q in levels], dtype=np.float64)


def rho(model, d2, range_):
    """The model's correlation of the distance sqrt(d2), in the contract's operations."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt(d2)
        r = d / range_
        r2 = r * r
        if model == 1:
            v = r * (1.5 - 0.5 * r2)
            return np.where(d < range_, 1.0 - v, np.where(d >= range_, 0.0, np.nan))
        return np.exp(-r2) if model == 2 else np.exp(-r)


def _table(what, nbr_idx, nbr_d2, k):
    nbr_idx = np.asarray(nbr_idx)
    if nbr_idx.ndim != 3 or (nbr_d2 is not None and np.shape(nbr_d2) != nbr_idx.shape):
        raise ValueError(f"{what}: the table must be (nM, M, k_tab)")
    k = int(k)
    if not 1 <= k <= nbr_idx.shape[2] <= MAX_K:
        raise ValueError(f"{what}: k={k} must be in 1..k_tab={nbr_idx.shape[2]} <= {MAX_K}")
    return nbr_idx.astype(np.int64), k


def row_groups(idx, c64):
    """Of rows idx (R, k) against coords c64 (S, 2) float64: counts (R, k), the pairwise d2 (R, k, k), rep (R, k) the
    first earlier coincident entry (itself for a first member) and members (R, k) the group size at a first member."""
    R, k = idx.shape
    S = len(c64)
    counts = (idx >= 0) & (idx < S)
    xy = c64[np.where(counts, idx, 0)] if S else np.zeros((R, k, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = xy[:, :, None, 0] - xy[:, None, :, 0], xy[:, :, None, 1] - xy[:, None, :, 1]
        dd = dx * dx + dy * dy
    rep = np.tile(np.arange(k), (R, 1))
    for e in range(k):
        for c in range(e):
            hit = counts[:, e] & counts[:, c] & (dd[:, e, c] == 0.0) & (rep[:, e] == e)
            rep[hit, e] = c
    members = np.zeros((R, k), dtype=np.int64)
    rows = np.arange(R)
    for c in range(k):
        at = counts[:, c]
        members[rows[at], rep[at, c]] += 1
    return counts, dd, rep, members


def _weights_block(idx, d0, c64, model, nugget, psill, range_):
    R, k = idx.shape
    counts, dd, rep, members = row_groups(idx, c64)
    lane = np.arange(k)
    act = counts & (rep == lane)
    both = act[:, :, None] & act[:, None, :]
    s = np.where(both, psill * rho(model, dd, range_), 0.0)
    own = nugget / np.where(members > 0, members, 1).astype(np.float64)
    s[:, lane, lane] = np.where(act, psill + own, 1.0)
    kk = np.where(act, psill * rho(model, d0, range_), 0.0)
    r1, rk = act.astype(np.float64), kk.copy()
    u_row, pivot = np.zeros((R, k, k)), np.ones((R, k))
    bad = np.zeros(R, dtype=bool)
    for c in range(k):                            # K = L L^T, and L y = (1, k) with it
        piv = s[:, c, c]
        bad |= act[:, c] & ~((piv > 0.0) & (piv < np.inf))
        p = np.sqrt(piv)
        pivot[:, c] = p
        l = s[:, :, c] / p[:, None]
        y1, yk = r1[:, c] / p, rk[:, c] / p
        r1[:, c + 1:] = r1[:, c + 1:] - l[:, c + 1:] * y1[:, None]
        rk[:, c + 1:] = rk[:, c + 1:] - l[:, c + 1:] * yk[:, None]
        r1[:, c], rk[:, c] = y1, yk
        s[:, c + 1:, c + 1:] = s[:, c + 1:, c + 1:] - l[:, c + 1:, None] * l[:, None, c + 1:]
        u_row[:, c, c + 1:] = l[:, c + 1:]
    for c in range(k - 1, -1, -1):                # L^T x = y from the last unknown down
        x1, xk = r1[:, c] / pivot[:, c], rk[:, c] / pivot[:, c]
        r1[:, :c] = r1[:, :c] - u_row[:, :c, c] * x1[:, None]
        rk[:, :c] = rk[:, :c] - u_row[:, :c, c] * xk[:, None]
        r1[:, c], rk[:, c] = x1, xk
    su, sv = np.zeros(R), np.zeros(R)
    for c in range(k):
        su, sv = su + r1[:, c], sv + rk[:, c]
    mu = (sv - 1.0) / su
    wt = rk - mu[:, None] * r1
    prod = np.where(act, wt * kk, 0.0)
    swk = np.zeros(R)
    for c in range(k):
        swk = swk + prod[:, c]
    var = ((nugget + psill) - swk) - mu
    rows = np.arange(R)[:, None]
    w = np.where(counts, wt[rows, rep] / np.where(members[rows, rep] > 0, members[rows, rep], 1).astype(np.float64), 0.0)
    w[bad] = np.nan
    var = np.where(bad | ~act.any(axis=1), np.nan, var)
    return w, var


def kriging_weights_host(nbr_idx, nbr_d2, k, coords, model, nugget, psill, range):      # noqa: A002
    """stdadk_krige_weights_f64 in numpy float64: the table nbr_idx / nbr_d2 (nM, M, k_tab), its first k entries, the
    sites coords (S, 2) float32, the model (a name or its code) and its parameters.  Returns w (nM, M, k) and var
    (nM, M): per row the ordinary-kriging weights (coincident entries share their group's weight, entries that do not
    count get 0) and the variance of a new noisy observation; w = 0 / var = NaN where no entry counts, all NaN where a
    pivot is <= 0 or not finite."""
    idx, k = _table("kriging_weights", nbr_idx, nbr_d2, k)
    model = model_code(model)
    nugget, psill, range_ = check_params(nugget, psill, range)
    c64 = np.asarray(coords, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    nM, M, _ = idx.shape
    idx = idx[:, :, :k].reshape(nM * M, k)
    d0 = np.asarray(nbr_d2, dtype=np.float64)[:, :, :k].reshape(nM * M, k)
    w, var = np.zeros((nM * M, k)), np.zeros(nM * M)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r0 in _span(0, nM * M, _BLOCK_ROWS):
            r1 = min(nM * M, r0 + _BLOCK_ROWS)
            w[r0:r1], var[r0:r1] = _weights_block(idx[r0:r1], d0[r0:r1], c64, model, nugget, psill, range_)
    return w.reshape(nM, M, k), var.reshape(nM, M)


def kriging_apply_host(nbr_idx, w, var, k, z, zq):
    """stdadk_krige_apply_f32 in numpy float64: the weights w (nM, M, k) and variances var (nM, M) on the table nbr_idx
    (nM, M, k_tab), nM == 1 or nM == nT, applied to z (nT, S) float32; zq the Q standard-normal quantiles (0 for the
    mean).  Returns (nT, M, Q) float32: (float32)(p + zq sd) with p = sum w z over the entries that count in row order
    and sd = sqrt(max(var, 0)); NaN where var is NaN."""
    idx, k = _table("kriging_apply", nbr_idx, None, k)
    w, var = np.asarray(w, dtype=np.float64), np.asarray(var, dtype=np.float64)
    z32 = np.asarray(z, dtype=np.float32)
    zq = np.asarray(zq, dtype=np.float64).reshape(-1)
    nM, M, _ = idx.shape
    if z32.ndim != 2 or nM not in (1, z32.shape[0]) or w.shape != (nM, M, k) or var.shape != (nM, M):
        raise ValueError(f"kriging_apply: z must be (nT, S), nM={nM} 1 or nT, w (nM, M, k) and var (nM, M)")
    if not 1 <= len(zq) <= MAX_COLS or not np.isfinite(zq).all():
        raise ValueError(f"kriging_apply: 1..{MAX_COLS} finite quantiles, got {zq}")
    nT, S = z32.shape
    z64 = z32.astype(np.float64)
    rows = np.arange(nT)[:, None]
    p = np.zeros((nT, M))
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(k):
            i = np.broadcast_to(idx[:, :, e], (nT, M))
            ok = (i >= 0) & (i < S)
            zv = z64[rows, np.where(ok, i, 0)] if S else np.zeros((nT, M))
            p = np.where(ok, p + np.broadcast_to(w[:, :, e], (nT, M)) * zv, p)
        v = np.broadcast_to(var, (nT, M))
        sd = np.sqrt(np.where(v > 0.0, v, 0.0))
        out = (p[:, :, None] + zq[None, None, :] * sd[:, :, None]).astype(np.float32)
    return np.where(np.isnan(v)[:, :, None], np.float32(np.nan), out).astype(np.float32)


def device_kriging_weights(nbr_idx, nbr_d2, k, coords, model, nugget, psill, range):      # noqa: A002
    """One stdadk_krige_weights_f64 call on device tensors; returns (w, var) on the device."""
    from .. import _native as N
    nM, M, _ = nbr_idx.shape
    w = torch.empty((nM, M, int(k)), dtype=torch.float64, device=nbr_idx.device)
    var = torch.empty((nM, M), dtype=torch.float64, device=nbr_idx.device)
    N.krige_weights(nbr_idx, nbr_d2, k, coords, model_code(model), nugget, psill, range, w, var)
    return w, var
