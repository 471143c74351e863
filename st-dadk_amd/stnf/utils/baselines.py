"""Neighbour baselines: does the model beat the interpolator one would have written in ten lines?
(stdadk_knn_f32, stdadk_knn_apply_f32; include/stdadk.h)

Two baselines on the same masks as the model's scores: NEAREST, the value of the nearest observed training site at the
same time, and IDW, inverse-distance weighting over the k nearest observed training sites (w = d^-power).  Training
entries are scored leave-one-site-out, so a training site never predicts itself.  `grid_baselines` scores both with the
reduction `grid_scores` uses; `grid_scores(..., config={"baselines": True})` puts them next to the model's numbers as a
skill score, 1 - mse_model / mse_baseline: 0 is no better than the baseline, negative is worse.

The neighbour table -- per target the k nearest sources in the total order (d2, source index), an index and a squared
distance each -- is an output in its own right; `rasterize_nearest` is its k = 1 case with raster nodes as targets: the
step the reference's summary maps take through scipy.interpolate.griddata(method="nearest")
(scripts/train_st_interp.py:1265-1270, :2764-2769).

The tables come from the device library (a HIP device) or from `knn_host` / `knn_apply_host`, the same contracts in
numpy float64: the path of `device: cpu`.  The device search is brute force (`search="brute"`, the default) or
cell-binned (`search="cells"`, config key `baseline_search`): the same table bit for bit, the second without meeting
every pair, which is what a table per time slice otherwise costs.
"""
import numpy as np
import torch

from .predictions import SPLIT_NAMES, _grid_sums_host, _quantile_sums_host, _ratio, _split_metrics, quantile_diagnostics

MAX_K = 16                                      # STDADK_KNN_MAX_K of include/stdadk.h
_EMPTY = np.uint64(0x7FF0000000000001)          # the key of no neighbour: above +inf's bits, at or below every NaN's
_DEFAULT_ROWS = 1 << 20                         # rows (time slices x sites) per chunk when max_rows is not given
SEARCHES = ("brute", "cells")                   # stdadk_knn_f32, stdadk_knn_cells_f32: one table


def _check_method(who, search):
    if search not in SEARCHES:
        raise ValueError(f"{who}: search must be one of {SEARCHES}, got {search!r}")
    return search


def _keys(q, c):
    """The (M, S) squared distances of the contract as KEYS: d2 = dx dx + dy dy in float64 from the float32 operands,
    every operation rounded once, its bits read as uint64 (d2 is never negative and never -0, so unsigned order is
    numeric order, +inf included); a NaN d2 becomes _EMPTY."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = q[:, None, 0] - c[None, :, 0], q[:, None, 1] - c[None, :, 1]
        d2 = dx * dx + dy * dy
    key = np.ascontiguousarray(d2).view(np.uint64)
    key[np.isnan(d2)] = _EMPTY
    return key


def _check_search(q, coords, src, k, exclude_self):
    q = np.asarray(q, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    c = np.asarray(coords, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn: k={k} outside 1..{MAX_K}")
    if exclude_self and len(q) != len(c):
        raise ValueError(f"knn: exclude_self needs M == S, got M={len(q)}, S={len(c)}")
    if src is not None:
        src = np.asarray(src)
        if src.ndim != 2 or src.shape[1] != len(c):
            raise ValueError(f"knn: src must be (nM, S) with S={len(c)}, got {src.shape}")
        src = src != 0
    return q, c, src, k


def knn_host(q, coords, src=None, k=8, exclude_self=False, block_pairs=1 << 22):
    """stdadk_knn_f32 in numpy float64: q (M, 2) and coords (S, 2) float32, src (nM, S) (non-zero = a source of the
    slice) or None (every site, one slice).  Returns nbr_idx (nM, M, k) int32 and nbr_d2 (nM, M, k) float64: per target
    the k smallest sources in the total order (d2, index) -- np.lexsort((index, d2))[:k] -- in that order, a row short of
    k sources ending in -1 / +inf; a NaN d2 is never a neighbour; exclude_self (M == S) skips source j for target j.
    Targets are walked in blocks of about `block_pairs` pairs."""
    q, c, src, k = _check_search(q, coords, src, k, exclude_self)
    M, S = len(q), len(c)
    nM = 1 if src is None else src.shape[0]
    idx = np.full((nM, M, k), -1, dtype=np.int32)
    d2 = np.full((nM, M, k), np.inf)
    for m in range(nM):
        sel = np.arange(S) if src is None else np.nonzero(src[m])[0]      # ascending: a column order is the index order
        n = len(sel)
        if n == 0 or M == 0:
            continue
        cols = max(n, k)
        step = max(1, block_pairs // cols)
        for j0 in range(0, M, step):
            j1 = min(M, j0 + step)
            key = np.full((j1 - j0, cols), _EMPTY, dtype=np.uint64)
            key[:, :n] = _keys(q[j0:j1], c[sel])
            if exclude_self:
                at = np.searchsorted(sel, np.arange(j0, j1))
                hit = (at < n) & (sel[np.minimum(at, n - 1)] == np.arange(j0, j1))
                key[np.nonzero(hit)[0], at[hit]] = _EMPTY
            # the k-th smallest key t of a row: every key below it is in, and of the keys equal to it the lowest columns
            t = np.partition(key, k - 1, axis=1)[:, k - 1:k]
            below, equal = key < t, key == t
            room = k - below.sum(axis=1, keepdims=True)
            take = below | (equal & (np.cumsum(equal, axis=1) <= room))
            col = np.nonzero(take)[1].reshape(j1 - j0, k)                    # k per row, ascending columns
            kk = np.take_along_axis(key, col, axis=1)
            order = np.argsort(kk, axis=1, kind="stable")                    # equal keys keep the column order
            col, kk = np.take_along_axis(col, order, axis=1), np.take_along_axis(kk, order, axis=1)
            none = kk == _EMPTY
            idx[m, j0:j1] = np.where(none, -1, sel[np.minimum(col, n - 1)])
            d2[m, j0:j1] = np.where(none, np.inf, kk.view(np.float64))
    return idx, d2


def _weights(d2, power):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if power == 0:
            return np.ones_like(d2)
        if power == 1:
            return 1.0 / np.sqrt(d2)
        if power == 2:
            return 1.0 / d2
        if power == 3:
            return 1.0 / (d2 * np.sqrt(d2))
        return 1.0 / (d2 * d2)


def knn_apply_host(nbr_idx, nbr_d2, k, z, power=2):
    """stdadk_knn_apply_f32 in numpy float64: the table nbr_idx / nbr_d2 (nM, M, k_tab), nM == 1 or nM == nT, applied
    to z (nT, S) float32 with the first k entries of every row.  Returns nearest (nT, M) and idw (nT, M) float32: the
    value of the first entry that counts (0 <= idx < S); the mean of z over the leading run of zero distances where the
    row starts with one, otherwise sum(w z) / sum(w) with w = 1, 1/sqrt(d2), 1/d2, 1/(d2 sqrt(d2)), 1/(d2 d2) for power
    0..4, sequentially in row order, every operation rounded once; NaN where no entry counts."""
    nbr_idx, nbr_d2 = np.asarray(nbr_idx), np.asarray(nbr_d2, dtype=np.float64)
    z32 = np.asarray(z, dtype=np.float32)
    if nbr_idx.ndim != 3 or nbr_d2.shape != nbr_idx.shape or z32.ndim != 2:
        raise ValueError("knn_apply: the table must be (nM, M, k_tab) twice and z (nT, S)")
    nM, M, k_tab = nbr_idx.shape
    nT, S = z32.shape
    k, power = int(k), int(power)
    if nM not in (1, nT) or not 1 <= k <= k_tab <= MAX_K or not 0 <= power <= 4:
        raise ValueError(f"knn_apply: nM={nM} must be 1 or nT={nT}, k={k} in 1..k_tab={k_tab} <= {MAX_K}, power={power} in 0..4")
    z64 = z32.astype(np.float64)
    first = np.full((nT, M), -1, dtype=np.int64)
    zero, run = np.zeros((nT, M), dtype=bool), np.ones((nT, M), dtype=bool)
    num, den = np.zeros((nT, M)), np.zeros((nT, M))
    rows = np.arange(nT)[:, None]
    for e in range(k):
        i = np.broadcast_to(nbr_idx[:, :, e].astype(np.int64), (nT, M))
        d = np.broadcast_to(nbr_d2[:, :, e], (nT, M))
        ok = (i >= 0) & (i < S)
        zv = z64[rows, np.where(ok, i, 0)] if S else np.zeros((nT, M))
        is_first = ok & (first < 0)
        first = np.where(is_first, i, first)
        zero = np.where(is_first, d == 0.0, zero)
        run = np.where(ok & zero, run & (d == 0.0), run)
        mean = ok & zero & run
        rest = ok & ~zero
        w = _weights(d, power)
        with np.errstate(invalid="ignore", over="ignore"):
            num = np.where(mean, num + zv, np.where(rest, num + w * zv, num))
            den = np.where(mean, den + 1.0, np.where(rest, den + w, den))
    some = first >= 0
    nearest = np.where(some, z32[rows, np.where(some, first, 0)] if S else np.float32(0), np.float32(np.nan))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        idw = np.where(some, (num / den).astype(np.float32), np.float32(np.nan))
    return nearest.astype(np.float32), idw.astype(np.float32)


def _host(a):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)


def _hip(device):
    return device is not None and torch.device(device).type == "cuda"


def device_knn(q, coords, src, k, exclude_self, search="brute"):
    """One stdadk_knn_f32 call (`search="cells"`: stdadk_knn_cells_f32, the same table) on device tensors; returns the
    table (nbr_idx, nbr_d2) on the device."""
    from .. import _native as N
    sizer, call = (N.knn_workspace_bytes, N.knn) if _check_method("device_knn", search) == "brute" else \
        (N.knn_cells_workspace_bytes, N.knn_cells)
    M, S = q.shape[0], coords.shape[0]
    nM = 1 if src is None else src.shape[0]
    idx = torch.empty((nM, M, k), dtype=torch.int32, device=q.device)
    d2 = torch.empty((nM, M, k), dtype=torch.float64, device=q.device)
    ws = torch.empty(sizer(M, S, nM, k) // 8, dtype=torch.float64, device=q.device)
    call(q, coords, src, k, exclude_self, idx, d2, ws)
    return idx, d2


def _search(q, coords, src, k, exclude_self, device, search="brute"):
    """The table as host arrays, by the device library (either search) or by knn_host."""
    _check_method("search", search)
    if not _hip(device):
        return knn_host(q, coords, src, k, exclude_self)
    dev = torch.device(device)
    to = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    with torch.cuda.device(dev):
        idx, d2 = device_knn(to(q, np.float32), to(coords, np.float32), to(src, np.uint8), k, exclude_self, search)
        return idx.cpu().numpy(), d2.cpu().numpy()


def _codes(shape, train_mask, valid_mask, test_mask):
    """grid_scores' split codes: 1 / 2 / 3 for train / valid / test, 0 in none; the higher code wins."""
    code = np.zeros(shape, dtype=np.uint8)
    for c, mask in ((1, train_mask), (2, valid_mask), (3, test_mask)):
        if mask is not None:
            mask = _host(mask).astype(bool)
            if mask.shape != shape:
                raise ValueError(f"grid_baselines: mask of split {SPLIT_NAMES[c]} has shape {mask.shape}, z_full {shape}")
            code[mask] = c
    return code


def _entry(split_acc, site_acc, time_acc):
    out = {"splits": {"all": _split_metrics(split_acc.sum(axis=0), "mean", 1, False)}}
    for c in (1, 2, 3, 0):
        out["splits"][SPLIT_NAMES[c]] = _split_metrics(split_acc[c], "mean", 1, False)
    out["site_mse"] = _ratio(site_acc.sum(axis=0)[:, 0], site_acc.sum(axis=0)[:, 2])
    out["site_mse_by_split"] = _ratio(site_acc[:, :, 0], site_acc[:, :, 2])
    out["time_mse"] = _ratio(time_acc.sum(axis=0)[:, 0], time_acc.sum(axis=0)[:, 2])
    return out


def _kriging_plan(config, k, z, c, code, device):
    """What `baseline_kriging: true` asks for, from the config: the model and its parameters (given, or fitted to the
    lag-0 field variogram of the training entries), the neighbours, and the columns of the prediction buffer -- the mean
    as the level 0.5 among the ascending `kriging_levels`, so that the buffer is a quantile model's."""
    from . import kriging as KR
    from . import variogram as V
    model = str(config.get("kriging_model", "exponential"))
    code_m = KR.model_code(model)
    kk = int(config.get("kriging_k", k))
    if not 1 <= kk <= MAX_K:
        raise ValueError(f"grid_baselines: kriging_k={kk} outside 1..{MAX_K}")
    levels = [float(q) for q in config.get("kriging_levels") or []]
    if len(levels) > KR.MAX_COLS - 1 or any(b <= a for a, b in zip(levels, levels[1:])):
        raise ValueError(f"grid_baselines: kriging_levels must be at most {KR.MAX_COLS - 1} ascending levels, got {levels}")
    KR.normal_quantiles(levels)                   # (refuses a level outside (0, 1))
    mean_col = sum(q < 0.5 for q in levels)
    taus = levels[:mean_col] + [0.5] + levels[mean_col:]
    if config.get("kriging_params") is not None:
        nugget, psill, range_ = KR.check_params(*config["kriging_params"])
        fit = {"model": model, "nugget": nugget, "psill": psill, "range": range_, "wss": float("nan"), "bins_used": 0}
    else:
        curves = V.field_variogram(z, c, code=code, n_bins=config.get("variogram_bins", 15),
                                   max_dist=config.get("variogram_max_dist"), time_lags=1,
                                   sites=config.get("variogram_sites"), device=device)
        fit = V.fit_variogram(curves["gamma_z"][1, 0], curves["count"][1, 0], curves["edges"], model)
        KR.check_params(fit["nugget"], fit["psill"], fit["range"])
    return {"model": model, "code": code_m, "k": kk, "levels": levels, "taus": taus, "zq": KR.normal_quantiles(taus),
            "mean_col": mean_col, "interval": len(levels) >= 2, "fit": fit,
            "params": (fit["nugget"], fit["psill"], fit["range"])}


def _calibration_sums_host(pred, var, z, code):
    """(4, 3) per split code: the entries with a finite z, a finite prediction and a variance > 0, the sum of their
    variances and the sum of (z - prediction)^2 / variance."""
    p, zz = pred.astype(np.float64), z.astype(np.float64)
    v = np.broadcast_to(var, zz.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = np.isfinite(zz) & np.isfinite(p) & (v > 0.0) & np.isfinite(v)
        e2 = np.where(ok, (zz - p) ** 2 / np.where(ok, v, 1.0), 0.0)
    out = np.zeros((4, 3))
    for s in range(4):
        m = ok & (code == s)
        out[s] = m.sum(), np.where(m, v, 0.0).sum(), np.where(m, e2, 0.0).sum()
    return out


def _calibration_sums_device(pred, var, z, code):
    """_calibration_sums_host on device tensors: (4, 3) float64 on the device."""
    p, zz = pred.double(), z.double()
    v = var.expand_as(zz)
    ok = torch.isfinite(zz) & torch.isfinite(p) & (v > 0.0) & torch.isfinite(v)
    one = torch.ones((), dtype=torch.float64, device=z.device)
    e2 = torch.where(ok, (zz - p) ** 2 / torch.where(ok, v, one), 0.0 * one)
    out = torch.zeros((4, 3), dtype=torch.float64, device=z.device)
    for s in range(4):
        m = ok & (code == s)
        out[s, 0], out[s, 1], out[s, 2] = m.sum(), torch.where(m, v, 0.0 * one).sum(), torch.where(m, e2, 0.0 * one).sum()
    return out


def _kriging_entry(plan, accs, qd_split, cal, n_singular):
    out = _entry(*accs)
    out.update(model=plan["model"], k=plan["k"], nugget=plan["params"][0], psill=plan["params"][1],
               range=plan["params"][2], variogram_fit=plan["fit"], n_singular=int(n_singular), mean_var={}, msse={})
    cal = np.concatenate([cal.sum(axis=0, keepdims=True), cal])      # all, then the codes 0..3
    for name, row in zip(("all", "other", "train", "valid", "test"), cal):
        out["mean_var"][name], out["msse"][name] = float(_ratio(row[1], row[0])), float(_ratio(row[2], row[0]))
    if plan["levels"]:
        out["levels"] = np.asarray(plan["taus"], dtype=np.float64)
        diag = quantile_diagnostics(qd_split, None, None, plan["taus"], plan["interval"])
        for name, d in diag.items():
            out["splits"][name].update({key: d[key] for key in ("crps", "reliability", "coverage") if key in d})
    return out


def grid_baselines(z_full, coords, train_mask, valid_mask=None, test_mask=None, config=None, device=None, max_rows=None):
    """The two neighbour baselines of a (T, S) field scored like a model's grid (grid_scores): at every entry NEAREST is
    the value, at the same time, of the nearest source site and IDW the inverse-distance weighted mean of the
    `baseline_k` (8) nearest, w = d^-`baseline_power` (2; 0..4).  The SOURCES of a time slice are its entries with
    `train_mask` set and a finite z; a site is never its own source (leave-one-site-out), so training entries are scored
    honestly too.  An entry with no source at its time has no prediction; it counts as a NaN prediction would.

    If the source set is the same at every time (the reference's site-wise observation and split methods) ONE table
    serves the whole grid; otherwise a table per time slice, in chunks of at most `max_rows` rows (time slices x
    sites): one brute-force search per slice, which is what the per-time route costs.  `baseline_per_time: true` forces
    that route.  `baseline_search`: "brute" (default) or "cells" -- every device search of the call (the shared table,
    the per-time chunks, `train_dist`) through stdadk_knn_cells_f32, the same tables bit for bit; the host route ignores
    it.  `device`: a HIP device runs stdadk_knn_f32 / stdadk_knn_apply_f32 and scores each chunk's two
    predictions with stdadk_grid_score_f32 into float64 accumulators read ONCE; otherwise numpy float64 on the host.

    Returns {"nearest": e, "idw": e, "k", "power", "shared_table", "train_dist"} with e = {"splits": grid_scores' metric
    dict per split (all, train, valid, test, other), "site_mse" (S,), "site_mse_by_split" (4, S), "time_mse" (T,)} and
    `train_dist` (S,) the distance from every site to the nearest OTHER site with any training observation (inf when
    there is none).

    `baseline_kriging: true` adds a third entry, `kriging`: local ordinary kriging over the `kriging_k` (default
    `baseline_k`) nearest sources of the same tables, under ONE variogram model `kriging_model` (exponential, spherical,
    gaussian) -- `kriging_params` (nugget, psill, range), or else fitted by `fit_variogram` to the lag-0 field variogram
    of the training entries (one `field_variogram` call with the `variogram_*` keys' defaults).  The weights are solved
    once per table; the kriging variance (of a new noisy observation) makes the baseline probabilistic:
    `kriging_levels` (ascending, at most 7) adds the Gaussian quantiles prediction + z_tau sd as columns, the mean among
    them as level 0.5, and the per-split dicts gain `crps`, `reliability` and, with two levels or more, the `coverage`
    of the interval between the lowest and the highest.  The entry has the shape of the other two plus `model`, `k`,
    `nugget`, `psill`, `range`, `variogram_fit`, `n_singular` (table rows with sources whose system was singular: no
    prediction there), and per split `mean_var` and `msse`, the mean of (z - prediction)^2 / variance over the entries
    with a prediction and a variance > 0: about 1 when the variogram is right.  The nugget is on the diagonal only, so
    the prediction is of the smooth signal.  Not built: universal and space-time kriging, anisotropy, a global solve,
    covariates."""
    config = config or {}
    z = _host(z_full).astype(np.float32)
    c = _host(coords).astype(np.float32)
    if z.ndim != 2 or c.shape != (z.shape[1], 2):
        raise ValueError(f"grid_baselines: z_full must be (T, S) and coords (S, 2), got {z.shape} and {c.shape}")
    T, S = z.shape
    if train_mask is None:
        raise ValueError("grid_baselines: the training mask names the sources")
    code = _codes((T, S), train_mask, valid_mask, test_mask)
    k, power = int(config.get("baseline_k", 8)), int(config.get("baseline_power", 2))
    if not 1 <= k <= MAX_K or not 0 <= power <= 4:
        raise ValueError(f"grid_baselines: baseline_k={k} outside 1..{MAX_K} or baseline_power={power} outside 0..4")
    search = _check_method("grid_baselines: baseline_search", config.get("baseline_search", "brute"))
    src = (_host(train_mask).astype(bool) & np.isfinite(z)).astype(np.uint8)
    plan = _kriging_plan(config, k, z, c, code, device) if config.get("baseline_kriging", False) and S and T else None
    k_tab = max(k, plan["k"]) if plan else k
    nB = 3 if plan else 2
    Qk = len(plan["taus"]) if plan else 0
    cal, qd_split, n_singular = np.zeros((4, 3)), None, 0
    shared = T > 0 and bool((src == src[:1]).all()) and not config.get("baseline_per_time", False)
    per = max(1, min(T, (int(max_rows) if max_rows else _DEFAULT_ROWS) // max(S, 1)))
    any_src = src.any(axis=0, keepdims=True).astype(np.uint8)
    accs = [[np.zeros((4, 16)), np.zeros((4, S, 3)), np.zeros((4, T, 3))] for _ in range(nB)]
    train_d2 = np.full(S, np.inf)
    if S == 0 or T == 0:
        pass
    elif _hip(device):
        from .. import _native as N
        dev = torch.device(device)
        with torch.cuda.device(dev):
            f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)      # noqa: E731
            ct, zt, st, codet = (torch.from_numpy(a).to(dev) for a in (c, z, src, code))
            near_d2 = device_knn(ct, ct, torch.from_numpy(any_src).to(dev), 1, True, search)[1].reshape(S)
            dacc = [(f64(4, N.GRID_SLOTS), f64(4, S, 3), f64(4, T, 3)) for _ in range(nB)]
            table = device_knn(ct, ct, st[:1], k_tab, True, search) if shared else None
            ws = torch.empty(N.grid_score_workspace_bytes(S, per) // 8, dtype=torch.float64, device=dev)
            extra = ()
            if plan:
                from .kriging import device_kriging_weights
                solve = lambda tab: device_kriging_weights(tab[0], tab[1], plan["k"], ct, plan["code"], *plan["params"])      # noqa: E731
                singular = lambda tab, var: (torch.isnan(var) & (tab[0][:, :, 0] >= 0)).sum().double().reshape(1)      # noqa: E731
                dcal, dsing = f64(4, 3), f64(1)
                dqd = f64(4, N.QD_SLOTS) if plan["levels"] else f64(0)
                qws = torch.empty(N.quantile_diag_workspace_bytes(S, per) // 8, dtype=torch.float64, device=dev) \
                    if plan["levels"] else None
                if shared:
                    wk, vk = solve(table)
                    dsing += singular(table, vk)
            for t0 in range(0, T, per):
                n = min(per, T - t0)
                idx, d2 = table if shared else device_knn(ct, ct, st[t0:t0 + n], k_tab, True, search)
                if plan:
                    if not shared:
                        wk, vk = solve((idx, d2))
                        dsing += singular((idx, d2), vk)
                    predk = torch.empty((n * S, Qk), dtype=torch.float32, device=dev)
                    N.krige_apply(idx, wk, vk, plan["k"], zt[t0:t0 + n], plan["zq"], predk)
                    tacc = f64(4, n, 3)
                    N.grid_score(predk, zt[t0:t0 + n], codet[t0:t0 + n], plan["mean_col"], plan["taus"],
                                 0 if plan["interval"] else -1, Qk - 1 if plan["interval"] else -1,
                                 dacc[2][0], dacc[2][1], tacc, ws)
                    dacc[2][2][:, t0:t0 + n] = tacc
                    if plan["levels"]:
                        N.quantile_diag(predk, zt[t0:t0 + n], codet[t0:t0 + n], plan["taus"],
                                        0 if plan["interval"] else -1, Qk - 1 if plan["interval"] else -1, dqd, None, None, qws)
                    dcal += _calibration_sums_device(predk[:, plan["mean_col"]].reshape(n, S), vk, zt[t0:t0 + n],
                                                     codet[t0:t0 + n])
                pred = torch.empty((2, n, S), dtype=torch.float32, device=dev)
                N.knn_apply(idx, d2, k, zt[t0:t0 + n], power, pred[0], pred[1])
                for b in range(2):
                    tacc = f64(4, n, 3)
                    N.grid_score(pred[b].reshape(n * S, 1), zt[t0:t0 + n], codet[t0:t0 + n], 0, None, -1, -1,
                                 dacc[b][0], dacc[b][1], tacc, ws)
                    dacc[b][2][:, t0:t0 + n] = tacc
            if plan:
                extra = (dcal, dsing, dqd)
            flat = torch.cat([a.reshape(-1) for a in sum(dacc, (near_d2,)) + extra]).cpu().numpy()      # the ONE host read
        train_d2, flat = flat[:S], flat[S:]
        for b in range(nB):
            for i, a in enumerate(accs[b]):
                accs[b][i], flat = flat[:a.size].reshape(a.shape), flat[a.size:]
        if plan:
            cal, n_singular, qd_split = flat[:12].reshape(4, 3), flat[12], flat[13:].reshape(4, -1)
    else:
        train_d2 = knn_host(c, c, any_src, 1, True)[1].reshape(S)
        table = knn_host(c, c, src[:1], k_tab, True) if shared else None
        if plan:
            from .kriging import kriging_apply_host, kriging_weights_host
            solve = lambda tab: kriging_weights_host(tab[0], tab[1], plan["k"], c, plan["code"], *plan["params"])      # noqa: E731
            singular = lambda tab, var: int((np.isnan(var) & (tab[0][:, :, 0] >= 0)).sum())      # noqa: E731
            qd_split = np.zeros((4, 32))
            lo, hi = (0, Qk - 1) if plan["interval"] else (-1, -1)
            if shared:
                wk, vk = solve(table)
                n_singular += singular(table, vk)
        for t0 in range(0, T, per):
            n = min(per, T - t0)
            idx, d2 = table if shared else knn_host(c, c, src[t0:t0 + n], k_tab, True)
            if plan:
                if not shared:
                    wk, vk = solve((idx, d2))
                    n_singular += singular((idx, d2), vk)
                predk = kriging_apply_host(idx, wk, vk, plan["k"], z[t0:t0 + n], plan["zq"])
                mc = plan["mean_col"]
                sp, si, ti = _grid_sums_host(predk[:, :, mc:mc + 1], z[t0:t0 + n], code[t0:t0 + n], None, -1, -1)
                accs[2][0] += sp
                accs[2][1] += si
                accs[2][2][:, t0:t0 + n] = ti
                if plan["levels"]:
                    # (the levels as the device takes them: float32)
                    qd_split += _quantile_sums_host(predk, z[t0:t0 + n], code[t0:t0 + n],
                                                    np.asarray(plan["taus"], dtype=np.float32).astype(np.float64), lo, hi)[0]
                cal += _calibration_sums_host(predk[:, :, mc], vk, z[t0:t0 + n], code[t0:t0 + n])
            for b, pred in enumerate(knn_apply_host(idx, d2, k, z[t0:t0 + n], power)):
                sp, si, ti = _grid_sums_host(pred[:, :, None], z[t0:t0 + n], code[t0:t0 + n], None, -1, -1)
                accs[b][0] += sp
                accs[b][1] += si
                accs[b][2][:, t0:t0 + n] = ti
    out = {"nearest": _entry(*accs[0]), "idw": _entry(*accs[1]), "k": k, "power": power, "shared_table": shared,
           "train_dist": np.sqrt(train_d2)}
    if plan:
        out["kriging"] = _kriging_entry(plan, accs[2], qd_split, cal, n_singular)
    return out


def skill_scores(model_scores, baseline):
    """What grid_scores adds to grid_baselines' dict: `skill` {baseline: {split: 1 - mse_model / mse_baseline}} and
    `site_skill` (2, S), the same ratio per site on the test split, rows nearest, idw -- and kriging, a third name and a
    third row, when the dict has that entry.  NaN where either MSE is NaN or the baseline's is 0.  A skill of 0 is no better than the baseline, a negative skill is worse, 1 is a perfect model."""
    def skill(model_mse, base_mse):
        model_mse, base_mse = np.asarray(model_mse, dtype=np.float64), np.asarray(base_mse, dtype=np.float64)
        ok = np.isfinite(model_mse) & np.isfinite(base_mse) & (base_mse != 0)
        return np.where(ok, 1.0 - model_mse / np.where(ok, base_mse, 1.0), np.nan)
    names = ("nearest", "idw") + (("kriging",) if "kriging" in baseline else ())
    return {"skill": {b: {s: float(skill(m["mse"], baseline[b]["splits"][s]["mse"]))
                          for s, m in model_scores["splits"].items()} for b in names},
            "site_skill": np.stack([skill(model_scores["site_mse_by_split"][3], baseline[b]["site_mse_by_split"][3])
                                    for b in names])}


def rasterize_nearest(coords, values, resolution=200, bounds=(0, 1), device=None, search="brute"):
    """Per-site values on a raster by the nearest site: coords (S, 2), values (S,) or (C, S); `resolution` n or
    (ny, nx); `bounds` (lo, hi) for both axes or ((x_lo, x_hi), (y_lo, y_hi)).  The nodes are np.linspace over the
    bounds as float32, in row-major `meshgrid` order (node [iy, ix] = (x[ix], y[iy])); the sources of a row of `values`
    are the sites where it is finite; ties go to the lower site index.  Returns (raster, x, y): raster (C, ny, nx), or
    (ny, nx) for one-dimensional values, float32, NaN where a row has no finite value.  This is the reference's
    griddata(..., method="nearest") step for its averaged-MSE and observation-density maps, as one k = 1 search on the
    device (`device`: a HIP device; `search`: "brute" or "cells", the same raster) or knn_host."""
    _check_method("rasterize_nearest", search)
    c = _host(coords).astype(np.float32)
    v = _host(values).astype(np.float32)
    one = v.ndim == 1
    v = v.reshape(1, -1) if one else v
    if c.ndim != 2 or c.shape[1] != 2 or v.ndim != 2 or v.shape[1] != len(c):
        raise ValueError(f"rasterize_nearest: coords must be (S, 2) and values (S,) or (C, S), got {c.shape} and {v.shape}")
    ny, nx = (int(resolution),) * 2 if np.ndim(resolution) == 0 else (int(r) for r in resolution)
    bx, by = (bounds, bounds) if np.ndim(bounds[0]) == 0 else bounds
    x = np.linspace(float(bx[0]), float(bx[1]), nx).astype(np.float32)
    y = np.linspace(float(by[0]), float(by[1]), ny).astype(np.float32)
    xg, yg = np.meshgrid(x, y)
    nodes = np.stack([xg.reshape(-1), yg.reshape(-1)], axis=1)
    fin = np.isfinite(v)
    if fin.all():                                  # one table serves every row
        idx = np.broadcast_to(_search(nodes, c, None, 1, False, device, search)[0], (len(v), ny * nx, 1))
    else:
        idx = _search(nodes, c, fin.astype(np.uint8), 1, False, device, search)[0]
    idx = idx[:, :, 0]
    some = idx >= 0
    raster = np.where(some, np.take_along_axis(v, np.where(some, idx, 0), axis=1) if len(c) else np.float32(0),
                      np.float32(np.nan)).astype(np.float32).reshape(len(v), ny, nx)
    return (raster[0] if one else raster), x, y
