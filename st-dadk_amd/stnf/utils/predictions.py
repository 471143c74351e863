"""Dense-grid predictions of a trained model and their `predictions.npz` record.

The reference's driver evaluates the model at every site for every time index, one `model(...)` call per time
slice (scripts/train_st_interp.py:1228-1248: `t = t_idx / (T - 1)` or 0 when T == 1, no covariates, the MEDIAN
quantile column of a multi-quantile model), and stores the (T, S) array next to the observed field and the three
masks (scripts/train_st_interp.py:2551-2560).  Here the same grid is one `Predictor.predict_grid` call on the
device (layer 0 once per site and once per time instead of once per (site, time)); on host tensors the model's own
forward runs time slice by time slice like the reference.
"""
import os

import numpy as np
import torch

NPZ_KEYS = ("predictions", "true", "coords", "train_mask", "valid_mask", "test_mask")
SPLIT_NAMES = ("other", "train", "valid", "test")          # split codes 0..3 of grid_scores
# slots per split of the sums behind grid_scores (the STDADK_GRID_* slots of include/stdadk.h)
_G_N, _G_SSE, _G_SAE, _G_COVER, _G_WIDTH, _G_CHECK, _G_SLOTS = 0, 1, 2, 3, 4, 5, 16
# slots per split of the sums behind the `quantile` entry of grid_scores (the STDADK_QD_* slots of include/stdadk.h)
_Q_N, _Q_BELOW, _Q_PIT, _Q_CROSS, _Q_PAIR, _Q_DEPTH1, _Q_DEPTH2, _Q_CRPS, _Q_INSIDE, _Q_SLOTS = \
    0, 1, 9, 18, 19, 26, 27, 28, 29, 32


@torch.no_grad()
def predict_all_times(model, coords, T, max_rows=None):
    """(T, S) float64 array of predictions at the S sites `coords` (ndarray or tensor, (S, 2)) for the time indices
    0 .. T-1 (normalised t = t_idx / (T - 1), 0.0 when T == 1); multi-output models contribute their median column
    output_dim // 2 (scripts/train_st_interp.py:1240-1245).  Runs under eval() and restores the mode."""
    if getattr(model, "p", 0) != 0:
        raise ValueError("predict_all_times: the dense grid has no covariates (p must be 0)")
    dev = next(model.parameters()).device
    c = torch.as_tensor(np.asarray(coords) if not torch.is_tensor(coords) else coords).float().to(dev)
    if c.dim() != 2 or c.shape[1] != 2:
        raise ValueError(f"predict_all_times: coords must be (S, 2), got {tuple(c.shape)}")
    T = int(T)
    S = c.shape[0]
    tv = torch.arange(T, dtype=torch.float32) / (T - 1) if T > 1 else torch.zeros(1, dtype=torch.float32)
    was_training = model.training
    model.eval()
    try:
        if dev.type == "cuda":
            from ..engine import Predictor
            out = Predictor(model).predict_grid(c, tv.to(dev), max_rows=max_rows)        # (T, S, Q)
        else:
            out = torch.stack([model(torch.zeros(S, 0), c, torch.full((S, 1), float(tv[i]))) for i in range(T)])
    finally:
        model.train(was_training)
    q = out.shape[2]
    col = out[:, :, q // 2] if q > 1 else out[:, :, 0]
    return col.double().cpu().numpy()


def save_predictions_npz(output_dir, predictions, true, coords, train_mask, valid_mask, test_mask):
    """Writes `<output_dir>/predictions.npz` with the reference's keys (scripts/train_st_interp.py:2551-2560) and
    returns its path.  Shapes are checked: predictions / true / masks (T, S), coords (S, 2)."""
    predictions = np.asarray(predictions)
    T, S = predictions.shape
    arrs = dict(predictions=predictions, true=np.asarray(true), coords=np.asarray(coords),
                train_mask=np.asarray(train_mask), valid_mask=np.asarray(valid_mask), test_mask=np.asarray(test_mask))
    for k in ("true", "train_mask", "valid_mask", "test_mask"):
        if arrs[k].shape != (T, S):
            raise ValueError(f"save_predictions_npz: {k} has shape {arrs[k].shape}, predictions {(T, S)}")
    if arrs["coords"].shape != (S, 2):
        raise ValueError(f"save_predictions_npz: coords has shape {arrs['coords'].shape}, expected {(S, 2)}")
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(str(output_dir), "predictions.npz")
    np.savez(path, **arrs)
    return path


@torch.no_grad()
def evaluate_model(model, dataset, config=None, predictor=None):
    """The driver's `evaluate_model` (scripts/train_st_interp.py:884-961) on a `DeviceDataset` (or any object with
    `.coords (N,2)`, `.t (N,1)`, `.y (N,1)`): predictions of the whole set under eval(), then on the host, in the
    reference's float32 numpy arithmetic: 'mse', 'mae', 'rmse' (of the median column for 'multi-quantile'), plus
    'check_loss' for `regression_type == 'quantile'` with `current_quantile`, and 'crps', 'mean_check_loss' and the
    'check_loss' alias for 'multi-quantile'.  The reference walks a DataLoader in batches of min(max(16 B, 32768), N)
    (:2292-2293); the predictions do not depend on the batching, so the set goes through `Predictor.predict` in
    its own chunks (device models) or one forward (host models).  `predictor`: reuse one across calls."""
    from ..losses import check_loss_numpy, compute_crps_multi_quantile      # host arithmetic (the predictions are small)
    dev = next(model.parameters()).device
    was_training = model.training
    model.eval()
    try:
        if dev.type == "cuda":
            if predictor is None:
                from ..engine import Predictor
                predictor = Predictor(model)
            preds_t = predictor.predict(dataset.coords, dataset.t)
        else:
            n = dataset.coords.shape[0]
            preds_t = model(torch.zeros(n, 0), dataset.coords, dataset.t.view(-1, 1))
    finally:
        model.train(was_training)
    pred = preds_t.float().cpu().numpy()                        # (N, Q) float32, like the reference's stacked batches
    obs = dataset.y.float().cpu().numpy().reshape(-1, 1)
    kind = (config or {}).get("regression_type", "mean")
    levels = list((config or {}).get("quantile_levels", [0.1, 0.5, 0.9])) if kind == "multi-quantile" else None
    # point metrics: the single output, or the median level's column of a multi-quantile head
    point = pred[:, len(levels) // 2:len(levels) // 2 + 1] if levels is not None else pred
    err = point - obs
    sq = float(np.mean(err * err))
    out = {"mse": sq, "mae": float(np.mean(np.abs(err))), "rmse": float(np.sqrt(np.mean(err * err)))}
    if kind == "quantile" and "current_quantile" in config:
        out["check_loss"] = float(check_loss_numpy(pred, obs, config["current_quantile"]))
    if levels is not None:
        per_level = [float(check_loss_numpy(pred[:, j:j + 1], obs, tau)) for j, tau in enumerate(levels)]
        out["crps"] = float(compute_crps_multi_quantile(pred, obs, levels))
        out["mean_check_loss"] = out["check_loss"] = float(np.mean(per_level))      # the reference keeps both names
    if (config or {}).get("conformal", False):
        # `dataset` is the calibration split: a Calibration from the predictions this pass made (stnf.calibration; the
        # interval of `interval`, at `conformal_alpha`, default its nominal miscoverage, otherwise 0.1)
        from ..calibration import calibrate_rows
        iv = config.get("interval") if levels is not None else None
        alpha = config.get("conformal_alpha", 0.1 if iv is None else round(1.0 - (float(iv[1]) - float(iv[0])), 12))
        target = dataset.y.float().reshape(pred.shape[0], -1)
        if levels is None and kind == "quantile" and "current_quantile" in config:
            levels = [float(config["current_quantile"])]
        out["calibration"] = calibrate_rows(preds_t.detach().float(), target[:, target.shape[1] // 2], levels,
                                            [iv] if iv is not None else None, alpha,
                                            split=str(config.get("conformal_split", "valid")))
    return out


def _grid_times(T):
    return torch.arange(T, dtype=torch.float32) / (T - 1) if T > 1 else torch.zeros(1, dtype=torch.float32)


def _grid_sums_host(pred, z, code, levels, lo, hi):
    """The sums of stdadk_grid_score_f32 in numpy float64: pred (T, S, Q), z (T, S) with NaN = no value, code (T, S)."""
    T, S, Q = pred.shape
    pred = pred.astype(np.float64)
    z = z.astype(np.float64)
    fin = np.isfinite(z)
    zz = np.where(fin, z, 0.0)
    d = pred[:, :, Q // 2] - zz
    split_acc, site_acc, time_acc = np.zeros((4, _G_SLOTS)), np.zeros((4, S, 3)), np.zeros((4, T, 3))
    for c in range(4):
        m = fin & (code == c)
        terms = np.stack([np.where(m, d * d, 0.0), np.where(m, np.abs(d), 0.0), m.astype(np.float64)], axis=2)
        site_acc[c], time_acc[c] = terms.sum(axis=0), terms.sum(axis=1)
        split_acc[c, [_G_SSE, _G_SAE, _G_N]] = terms.sum(axis=(0, 1))
        for q in range(Q):
            tau = 0.5 if levels is None else levels[q]
            e = zz - pred[:, :, q]
            split_acc[c, _G_CHECK + q] = np.where(m, np.maximum((tau - 1.0) * e, tau * e), 0.0).sum()
        if lo >= 0:
            split_acc[c, _G_COVER] = (m & (pred[:, :, lo] <= zz) & (zz <= pred[:, :, hi])).sum()
            split_acc[c, _G_WIDTH] = np.where(m, pred[:, :, hi] - pred[:, :, lo], 0.0).sum()
    return split_acc, site_acc, time_acc


def _quantile_sums_host(pred, z, code, levels, lo, hi):
    """The sums of stdadk_quantile_diag_f32 in numpy float64: pred (T, S, Q), z (T, S) with NaN = no value, code (T, S).
    Returns split_acc (4, slots), site_acc (4, S, 4), time_acc (4, T, 4); site and time hold (n, crps, cross_rows,
    inside)."""
    T, S, Q = pred.shape
    pred = pred.astype(np.float64)
    z = z.astype(np.float64)
    fin = np.isfinite(z)
    zz = np.where(fin, z, 0.0)[:, :, None]
    tau = np.asarray([0.5] * Q if levels is None else levels, dtype=np.float64)
    e = zz - pred
    crps = (2.0 / Q) * np.maximum((tau - 1.0) * e, tau * e).sum(axis=2)
    below = zz <= pred
    rank = (pred < zz).sum(axis=2)
    pair = pred[:, :, :-1] > pred[:, :, 1:]
    depth = np.maximum(pred[:, :, :-1] - pred[:, :, 1:], 0.0)
    cross = pair.any(axis=2)
    inside = (pred[:, :, lo] <= zz[:, :, 0]) & (zz[:, :, 0] <= pred[:, :, hi]) if lo >= 0 else np.zeros((T, S), bool)
    split_acc, site_acc, time_acc = np.zeros((4, _Q_SLOTS)), np.zeros((4, S, 4)), np.zeros((4, T, 4))
    for c in range(4):
        m = fin & (code == c)
        terms = np.stack([m.astype(np.float64), np.where(m, crps, 0.0), (m & cross).astype(np.float64),
                          (m & inside).astype(np.float64)], axis=2)
        site_acc[c], time_acc[c] = terms.sum(axis=0), terms.sum(axis=1)
        split_acc[c, [_Q_N, _Q_CRPS, _Q_CROSS, _Q_INSIDE]] = terms.sum(axis=(0, 1))
        split_acc[c, _Q_BELOW:_Q_BELOW + Q] = (below & m[:, :, None]).sum(axis=(0, 1))
        split_acc[c, _Q_PIT:_Q_PIT + Q + 1] = np.bincount(rank[m], minlength=Q + 1)
        split_acc[c, _Q_PAIR:_Q_PAIR + Q - 1] = (pair & m[:, :, None]).sum(axis=(0, 1))
        split_acc[c, _Q_DEPTH1] = np.where(m[:, :, None], depth, 0.0).sum()
        split_acc[c, _Q_DEPTH2] = np.where(m[:, :, None], depth * depth, 0.0).sum()
    return split_acc, site_acc, time_acc


def _quantile_split_metrics(sums, levels, interval):
    Q = len(levels)
    n = sums[_Q_N]
    out = {"levels": np.asarray(levels, dtype=np.float64),
           "reliability": _ratio(sums[_Q_BELOW:_Q_BELOW + Q], n), "pit": _ratio(sums[_Q_PIT:_Q_PIT + Q + 1], n),
           "cross_rate": float(_ratio(sums[_Q_CROSS], n)), "pair_cross_rate": _ratio(sums[_Q_PAIR:_Q_PAIR + Q - 1], n),
           "nc_penalty_p1": float(_ratio(sums[_Q_DEPTH1], n)), "nc_penalty_p2": float(_ratio(sums[_Q_DEPTH2], n)),
           "crps": float(_ratio(sums[_Q_CRPS], n)), "rows": int(n)}
    if interval:
        out["coverage"] = float(_ratio(sums[_Q_INSIDE], n))
    return out


def quantile_diagnostics(split_acc, site_acc, time_acc, levels, interval):
    """The `quantile` entry of grid_scores from the sums of stdadk_quantile_diag_f32 (host arrays): per split (all,
    train, valid, test, other) levels, reliability (Q,), pit (Q+1,), cross_rate, pair_cross_rate (Q-1,), nc_penalty_p1,
    nc_penalty_p2, crps, rows and, with an interval, coverage; and, when the site and time sums are given, the maps
    over all finite entries site_crps, site_cross_rate, site_coverage, site_count (S,), time_* (T,),
    site_crps_by_split, time_crps_by_split (4, .).  NaN / 0 where a split, site or time has no finite entry."""
    out = {"all": _quantile_split_metrics(split_acc.sum(axis=0), levels, interval)}
    for k in (1, 2, 3, 0):
        out[SPLIT_NAMES[k]] = _quantile_split_metrics(split_acc[k], levels, interval)
    for name, acc in (("site", site_acc), ("time", time_acc)):
        if acc is None:
            continue
        tot = acc.sum(axis=0)
        out[f"{name}_crps"], out[f"{name}_cross_rate"] = _ratio(tot[:, 1], tot[:, 0]), _ratio(tot[:, 2], tot[:, 0])
        out[f"{name}_coverage"] = _ratio(tot[:, 3], tot[:, 0]) if interval else np.full(tot.shape[0], np.nan)
        out[f"{name}_count"] = tot[:, 0].astype(np.int64)
        out[f"{name}_crps_by_split"] = _ratio(acc[:, :, 1], acc[:, :, 0])
    return out


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def _split_metrics(sums, kind, Q, interval):
    n = sums[_G_N]
    mse = float(_ratio(sums[_G_SSE], n))
    out = {"mse": mse, "mae": float(_ratio(sums[_G_SAE], n)), "rmse": mse ** 0.5, "rows": int(n)}
    checks = [float(_ratio(sums[_G_CHECK + q], n)) for q in range(Q)]
    if kind == "quantile":
        out["check_loss"] = checks[0]
    elif kind == "multi-quantile":
        # compute_crps_multi_quantile with its default weights: 2 x sum_k (1/K) x check loss at level k
        out["crps"] = 2.0 * sum(c / Q for c in checks)
        out["mean_check_loss"] = out["check_loss"] = sum(checks) / Q
    if interval:
        out["coverage"] = float(_ratio(sums[_G_COVER], n))
        out["mean_width"] = float(_ratio(sums[_G_WIDTH], n))
    return out


@torch.no_grad()
def grid_scores(model, z_full, coords, train_mask=None, valid_mask=None, test_mask=None, config=None, max_rows=None):
    """What the reference's driver computes last (scripts/train_st_interp.py:1228-1252, :1378-1409, :2242): the (T, S)
    prediction grid of `predict_all_times` (t = t_idx / (T - 1), 0 when T == 1; the median column Q // 2) against the
    full field `z_full` (T, S; NaN = no value, such entries count nowhere), per split, per site and per time.

    Device models never hold the grid: `Predictor.score_grid` reduces it chunk by chunk (at most `max_rows` rows)
    into float64 sums on the device, read by the host ONCE.  Host models (`device: cpu`) run their own forward time
    slice by time slice and sum in numpy float64.  (The device takes the quantile levels as float32.)

    Masks are (T, S) booleans; an entry's split code is 1 / 2 / 3 for train / valid / test and 0 in none of them, and
    where masks overlap the HIGHER code wins (test over valid over train).  `config`: `regression_type`,
    `quantile_levels` / `current_quantile` as for evaluate_model, and optionally `interval = (lo_level, hi_level)`,
    two of the quantile levels, for coverage and width.  Returns a dict:
      splits            {name: metrics} for all / train / valid / test / other: evaluate_model's keys (mse, mae, rmse,
                        check_loss, and crps, mean_check_loss for several levels) plus rows, and with an interval
                        coverage, mean_width; NaN where a split has no finite entry
      site_mse, site_mae, site_count   (S,) over all finite entries (the reference's nanmean), NaN / 0 for an empty site
      time_mse, time_mae, time_count   (T,)
      site_mse_by_split, time_mse_by_split   (4, .), rows in the order of the codes: other, train, valid, test
    With `quantile_diagnostics: true` in the config and a model that has quantile levels, the dict gains `quantile`
    (see quantile_diagnostics): reliability, PIT histogram, crossing rates and depths, CRPS per split, and the per-site
    and per-time CRPS / crossing / coverage maps.  On the device that is one more reduction of the same chunk buffer
    (one forward per chunk) and still one host read; without the key nothing changes.
    With `variogram: true` the dict gains `variogram`: per split name (other, train, valid, test) the empirical
    space-time semivariograms count, gamma_z, gamma_pred, gamma_resid, each (L, B), of the field, of the metric column
    and of their residual, with `edges` and `lags` (utils.variogram).  Keys: `variogram_bins` (15),
    `variogram_max_dist` (half the diagonal of the coordinates' bounding box), `variogram_time_lags` (1: lag 0 only),
    `variogram_sites` (every site up to 4 096, then 4 096 drawn by a RandomState(0) of its own; 'all'; an index array).
    On the device that is one more pass over the chosen sites, one stdadk_variogram_f32 call and one more host read;
    without the key nothing changes.
    With `basis_diagnostics: true` the dict gains `basis`: utils.basis_diag.basis_diagnostics' dict at the same sites,
    the site weights being the training observations per site (`train_mask.sum(0)`) and the site value the test split's
    per-site MSE computed here; `basis_rho` overrides the support radius.  On the device that is two more library calls
    and one more host read; without the key nothing changes.
    With `conformal: true` the dict gains `conformal` (stnf.calibration.report): split-conformal calibration on the
    split `conformal_split` (default `valid`) at miscoverage `conformal_alpha` (default the nominal one of `interval`,
    1 - (hi - lo), otherwise 0.1), shown on the test split -- per quantile level the one-sided offset and the
    reliability before and after; for `interval` the CQR offset, n_cal, coverage and mean width before and after; for a
    mean model the half-width of |z - yhat| and its coverage; `overflow` and `rank_beyond_n` (too few calibration
    entries for this alpha: the offset is +inf) are reported, never hidden; `calibration` is the Calibration record to
    apply or save.  On the device the scores are compacted from the same chunk buffer (one forward per chunk), one
    select call and one more host read; without the key nothing changes.  The guarantee is marginal over entries
    exchangeable with the calibration split: with site-wise splits it holds for new sites drawn like the validation
    sites, not for every site.
    With `baselines: true` the dict gains `baseline` (utils.baselines.grid_baselines): the scores, on the same masks, of
    NEAREST (copy the nearest training site observed at that time) and IDW (inverse-distance weighting over the
    `baseline_k` (8) nearest, w = d^-`baseline_power` (2)), training entries leave-one-site-out, each with `splits`,
    `site_mse`, `site_mse_by_split`, `time_mse`; `train_dist` (S,), the distance to the nearest other training site;
    and `skill` {baseline: {split: 1 - mse_model / mse_baseline}} with `site_skill` (2, S), the same per site on the
    test split (rows nearest, idw).  How to read it: a skill of 0 means the model is no better than the baseline, a
    negative skill that it is WORSE than an interpolator of ten lines, 1 a perfect model; NaN where either MSE is NaN or
    the baseline's is 0.  A training mask that is the same at every time costs one neighbour search for the whole
    grid; otherwise one brute-force search per time slice (`train_mask` is needed either way).  Without the key nothing
    changes."""
    if getattr(model, "p", 0) != 0:
        raise ValueError("grid_scores: the dense grid has no covariates (p must be 0)")
    z = np.asarray(z_full.detach().cpu() if torch.is_tensor(z_full) else z_full)
    if z.ndim != 2:
        raise ValueError(f"grid_scores: z_full must be (T, S), got {z.shape}")
    T, S = z.shape
    code = np.zeros((T, S), dtype=np.uint8)
    for c, mask in ((1, train_mask), (2, valid_mask), (3, test_mask)):
        if mask is not None:
            mask = np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask, dtype=bool)
            if mask.shape != (T, S):
                raise ValueError(f"grid_scores: mask of split {SPLIT_NAMES[c]} has shape {mask.shape}, z_full {(T, S)}")
            code[mask] = c
    config = config or {}
    kind = config.get("regression_type", "mean")
    Q = int(model.output_dim)
    levels = None
    if kind == "multi-quantile":
        levels = [float(q) for q in config.get("quantile_levels", [0.1, 0.5, 0.9])]
    elif kind == "quantile" and "current_quantile" in config:
        levels = [float(config["current_quantile"])]
    if levels is not None and len(levels) != Q:
        raise ValueError(f"grid_scores: the model has {Q} outputs, config names {len(levels)} quantile levels")
    if kind == "quantile" and levels is None:
        kind = "mean"
    # quantile diagnostics: asked for by the config and only of a model that has quantile levels
    diag = bool(config.get("quantile_diagnostics", False)) and levels is not None
    interval = config.get("interval")
    lo = hi = -1
    if interval is not None:
        if levels is None or any(float(v) not in levels for v in interval):
            raise ValueError(f"grid_scores: interval {interval} must name two of the quantile levels {levels}")
        lo, hi = levels.index(float(interval[0])), levels.index(float(interval[1]))
        if lo >= hi:
            raise ValueError(f"grid_scores: interval {interval} must be (lower level, upper level)")
    dev = next(model.parameters()).device
    c = torch.as_tensor(np.asarray(coords) if not torch.is_tensor(coords) else coords).float().to(dev)
    if tuple(c.shape) != (S, 2):
        raise ValueError(f"grid_scores: coords must be ({S}, 2), got {tuple(c.shape)}")
    tv = _grid_times(T)
    cf = cf_plan = None
    if config.get("conformal", False):
        from .. import calibration as CF
        cf_split = str(config.get("conformal_split", "valid"))
        if cf_split not in SPLIT_NAMES[:3]:
            raise ValueError(f"grid_scores: conformal_split '{cf_split}' must be one of {SPLIT_NAMES[:3]} (test evaluates)")
        cf_codes = [SPLIT_NAMES.index(cf_split), 3]
        # the nominal miscoverage of the interval's two levels, unless the config names one
        cf_alpha = config.get("conformal_alpha", 0.1 if interval is None else
                              round(1.0 - (float(interval[1]) - float(interval[0])), 12))
        cf_plan = CF.make_plan(Q, levels, [interval] if interval is not None else None, cf_alpha)
        members = np.isfinite(z)
        cf_cap = max(int((members & (code == k)).sum()) for k in cf_codes)
    vg = None
    if config.get("variogram", False):
        from . import variogram as V
        vg_lags = V._check_lags(config.get("variogram_time_lags", 1))
        vg_edges, vg_e2 = V._check_edges(V.variogram_edges(c.cpu().numpy(), config.get("variogram_bins", 15),
                                                           config.get("variogram_max_dist")))
        vg_sites = V.select_sites(S, config.get("variogram_sites"))
    was_training = model.training
    model.eval()
    pr = None
    try:
        if dev.type == "cuda":
            from ..engine import Predictor
            pr, zt, ct = Predictor(model), torch.from_numpy(z.astype(np.float32)).to(dev), torch.from_numpy(code).to(dev)
            more = {}
            if cf_plan is not None:
                more["conformal"] = pr.conformal_pass(cf_cap, levels, [interval] if interval is not None else None,
                                                      cf_alpha, *cf_codes)
            accs = pr.score_grid(c, tv.to(dev), zt, ct, quantile_levels=levels, interval=interval, max_rows=max_rows,
                                 quantile=diag, **more)
            flat = torch.cat([a.reshape(-1) for a in accs]).cpu().numpy()              # the ONE host read
            cuts = np.cumsum([a.numel() for a in accs])[:-1]
            sums = [part.reshape(a.shape) for part, a in zip(np.split(flat, cuts), accs)]
            if cf_plan is not None:
                cf = pr.conformal_finish(more["conformal"], cf_split)                  # (and the calibration's own)
            if config.get("variogram", False):
                vg = pr.variogram_grid(c, tv.to(dev), zt, ct, edges=vg_edges, time_lags=vg_lags,
                                       sites=vg_sites)["acc"]                          # (and the variogram's own)
        else:
            pred = torch.stack([model(torch.zeros(S, 0), c, torch.full((S, 1), float(tv[i]))) for i in range(T)])
            pred = pred.double().numpy()
            sums = list(_grid_sums_host(pred, z, code, levels, lo, hi))
            if diag:
                sums += _quantile_sums_host(pred, z, code, levels, lo, hi)
            if cf_plan is not None:
                segments = CF.scores_numpy(pred.astype(np.float32), z.astype(np.float32), code, cf_plan.cols, cf_codes)
                cf = CF.report(cf_plan, CF.finish_host(cf_plan, segments), cf_split)
            if config.get("variogram", False):
                vg = V.variogram_sums_host(pred[:, vg_sites, Q // 2].astype(np.float32), z[:, vg_sites].astype(np.float32),
                                           code[:, vg_sites], c.numpy()[vg_sites], vg_e2, vg_lags)
        split_acc, site_acc, time_acc = sums[:3]
    finally:
        model.train(was_training)
    out = {"splits": {"all": _split_metrics(split_acc.sum(axis=0), kind, Q, interval is not None)}}
    for k in (1, 2, 3, 0):
        out["splits"][SPLIT_NAMES[k]] = _split_metrics(split_acc[k], kind, Q, interval is not None)
    for name, acc in (("site", site_acc), ("time", time_acc)):
        tot = acc.sum(axis=0)
        out[f"{name}_mse"], out[f"{name}_mae"] = _ratio(tot[:, 0], tot[:, 2]), _ratio(tot[:, 1], tot[:, 2])
        out[f"{name}_count"] = tot[:, 2].astype(np.int64)
        out[f"{name}_mse_by_split"] = _ratio(acc[:, :, 0], acc[:, :, 2])
    if diag:
        out["quantile"] = quantile_diagnostics(*sums[3:], levels, interval is not None)
    if vg is not None:
        curves = V.variogram_curves(vg, vg_edges, np.arange(vg_lags))
        out["variogram"] = {SPLIT_NAMES[k]: dict({name: curves[name][k] for name in
                                                  ("count", "gamma_z", "gamma_pred", "gamma_resid")},
                                                 edges=curves["edges"], lags=curves["lags"]) for k in (1, 2, 3, 0)}
    if cf is not None:
        out["conformal"] = cf
    if config.get("basis_diagnostics", False):
        from .basis_diag import basis_diagnostics
        out["basis"] = basis_diagnostics(model, c, train_mask=train_mask, config=config,
                                         site_value=out["site_mse_by_split"][3], rho=config.get("basis_rho"),
                                         predictor=pr)
    if config.get("baselines", False):
        from .baselines import grid_baselines, skill_scores
        out["baseline"] = grid_baselines(z, c.cpu().numpy(), train_mask, valid_mask, test_mask, config=config,
                                         device=dev if dev.type == "cuda" else None, max_rows=max_rows)
        out["baseline"].update(skill_scores(out, out["baseline"]))
    return out


def save_grid_scores_npz(output_dir, scores):
    """Writes `<output_dir>/grid_scores.npz` from the dict of grid_scores and returns its path: the per-site and
    per-time arrays under their own names, every split metric as the 0-d array `splits/<split>/<metric>`, and the
    quantile diagnostics, when present, as `quantile/<split>/<metric>` and `quantile/<map>`, and the variograms, when
    present, as `variogram/<split>/<name>`, and the basis diagnostics, when present, as `basis/<name>`, and the neighbour
    baselines, when present, as `baseline/...` (e.g. `baseline/idw/splits/test/mse`, `baseline/skill/idw/test`)."""
    arrs = {k: np.asarray(v) for k, v in scores.items()
            if k not in ("splits", "quantile", "variogram", "basis", "conformal", "baseline")}
    # the neighbour baselines, when present: `baseline/<name>`, nested dicts joined by `/`
    todo = [("baseline", scores["baseline"])] if "baseline" in scores else []
    while todo:
        name, v = todo.pop()
        if isinstance(v, dict):
            todo += [(f"{name}/{k}", w) for k, w in v.items()]
        else:
            arrs[name] = np.asarray(v)
    # the conformal calibration, when present: the record's fields as `conformal/<field>` (calibration.load_calibration_npz
    # reads them back from a file of their own, save_calibration_npz)
    if "conformal" in scores:
        from ..calibration import _NPZ
        for k in _NPZ:
            arrs[f"conformal/{k}"] = np.asarray(getattr(scores["conformal"]["calibration"], k))
    for name, metrics in scores["splits"].items():
        for k, v in metrics.items():
            arrs[f"splits/{name}/{k}"] = np.asarray(v)
    # the quantile diagnostics, when they were asked for: `quantile/<split>/<metric>` and `quantile/<map>`
    for name, v in scores.get("quantile", {}).items():
        if isinstance(v, dict):
            for k, w in v.items():
                arrs[f"quantile/{name}/{k}"] = np.asarray(w)
        else:
            arrs[f"quantile/{name}"] = np.asarray(v)
    for name, v in scores.get("variogram", {}).items():
        for k, w in v.items():
            arrs[f"variogram/{name}/{k}"] = np.asarray(w)
    for name, v in scores.get("basis", {}).items():
        arrs[f"basis/{name}"] = np.asarray(v)
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(str(output_dir), "grid_scores.npz")
    np.savez(path, **arrs)
    return path
