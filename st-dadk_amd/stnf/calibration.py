"""Split-conformal calibration of a trained model's quantiles, intervals and point predictions.

`quantile_diagnostics` says how wrong a model's quantiles are; this module does something about it.  Take the
conformity scores of a CALIBRATION split (by default the validation split), pick one order statistic of them, shift:
  * an interval (lo, hi) at miscoverage alpha -- conformalized quantile regression: score max(q_lo - y, y - q_hi),
    offset c = the k-th smallest score, k = ceil((n + 1)(1 - alpha)); the calibrated interval is [q_lo - c, q_hi + c];
  * one quantile column at level tau: score y - q, k = ceil((n + 1) tau); the calibrated quantile is q + c;
  * a mean model: score |y - yhat|, k = ceil((n + 1)(1 - alpha)); the interval is yhat -+ c.
With k <= n the shifted interval covers a NEW observation with probability >= 1 - alpha whatever the model learned;
with k > n (too few calibration scores for this alpha) the offset is +inf, reported as such, never hidden.

THE CAVEAT.  The guarantee is marginal and rests on EXCHANGEABILITY of the calibration scores with the new one.  With
`site-wise` splits the validation sites are whole sites drawn at random, so it holds for a new site drawn like the
validation sites, averaged over such sites -- not for every site, not per time, and not for sites unlike them (another
region, another network density).  With random observation-wise splits it holds for a held-out observation of the same
sites and times.  It says nothing under a shift between calibration and use.

On the device the scores are an ordered compaction (stdadk_conformal_scores_f32) and the order statistic an exact radix
select (stdadk_select_f32): include/stdadk.h holds both contracts, this module their numpy restatements -- used for
`device: cpu` models and by the tests -- the rank rule, and the `Calibration` record.
Not built: locally adaptive (per-site or per-time) offsets, weighted conformal, covariates on the grid path.
"""
import math
import os
from dataclasses import dataclass, field

import numpy as np
import torch

RESID, CQR, ABS = 0, 1, 2                    # the score kinds (STDADK_CONFORMAL_* of include/stdadk.h)
MAX_COLS, MAX_SEGMENTS, MAX_SELECT = 8, 2, 16
SELECT_BITS = 8                              # digit width of the radix select


# ---- the rank rule ----------------------------------------------------------------------------------------------

def conformal_rank(n, beta):
    """The 0-based rank of the order statistic at level `beta` among n scores: k = ceil((n + 1) * beta) with that one
    product in IEEE double (the expression the device evaluates), k below 1 taken as 1, rank k - 1; -1 when k > n
    (n = 0 included): not enough calibration data."""
    k = max(int(math.ceil(float(n + 1) * float(beta))), 1)
    return k - 1 if k <= n else -1


def interval_beta(alpha):
    """Interval (CQR) and absolute scores at miscoverage alpha: the level 1 - alpha."""
    return 1.0 - float(alpha)


def level_beta(tau):
    """A one-sided offset of the quantile at level tau: the level tau itself."""
    return float(tau)


# ---- the two contracts in numpy ---------------------------------------------------------------------------------

def scores_numpy(pred, z, code, cols, codes):
    """stdadk_conformal_scores_f32 restated: pred (..., Q), z (...) with non-finite = no value, code (...) or None
    (all 0), cols [(kind, col_a, col_b)], codes [split code per segment].  Returns per segment the (C, n_g) float32
    scores of its members in C order of the flattened entries (time-major then site), float32 arithmetic throughout."""
    pred = np.asarray(pred, dtype=np.float32)
    Q = pred.shape[-1]
    p = pred.reshape(-1, Q)
    zz = np.asarray(z, dtype=np.float32).reshape(-1)
    cc = np.zeros(zz.shape, dtype=np.uint8) if code is None else np.asarray(code).reshape(-1)
    fin = np.isfinite(zz)
    out = []
    for g in codes:
        m = fin & (cc == g)
        zm, pm = zz[m], p[m]
        seg = np.empty((len(cols), zm.size), dtype=np.float32)
        for c, (kind, a, b) in enumerate(cols):
            if kind == RESID:
                seg[c] = zm - pm[:, a]
            elif kind == CQR:
                seg[c] = np.maximum(pm[:, a] - zm, zm - pm[:, b])
            elif kind == ABS:
                seg[c] = np.abs(zm - pm[:, a])
            else:
                raise ValueError(f"unknown score kind {kind}")
        out.append(seg)
    return out


def select_keys(x):
    """The order-preserving unsigned keys of float32 values: -0 canonicalised to +0, then all bits of negatives and
    the sign bit of the others flipped."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = np.where(x == 0, np.uint32(0), x.view(np.uint32))
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def select_values(keys):
    """The inverse of select_keys."""
    keys = np.asarray(keys, dtype=np.uint32)
    bits = np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32)
    return bits.view(np.float32)


def select_numpy(x, rank):
    """stdadk_select_f32 restated for one selection: the rank-th smallest (0-based) of the finite float32 values x by
    radix select on select_keys -- per pass the histogram of the digit among the keys that match the prefix, the bin
    where the cumulative count crosses the remaining rank.  Returns (value float32, rank_used); (+inf, -1) for a rank
    outside 0..n-1."""
    keys = select_keys(np.asarray(x, dtype=np.float32).reshape(-1))
    rank = int(rank)
    if rank < 0 or rank >= keys.size:
        return np.float32(np.inf), -1
    prefix, left = 0, rank
    for p in range(32 // SELECT_BITS):
        shift = 32 - SELECT_BITS * (p + 1)
        digit = (keys >> np.uint32(shift)) & np.uint32((1 << SELECT_BITS) - 1)
        hist = np.bincount(digit, minlength=1 << SELECT_BITS)
        cum = np.cumsum(hist)
        d = int(np.searchsorted(cum, left, side="right"))
        left -= int(cum[d] - hist[d])
        prefix |= d << shift
        keys = keys[digit == d]
    return select_values(np.array([prefix], dtype=np.uint32))[0], rank


def select_level_numpy(x, beta):
    """select_numpy at the rank of conformal_rank(n, beta)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    return select_numpy(x, conformal_rank(x.size, beta))


# ---- what a calibration asks of the two calls -------------------------------------------------------------------

@dataclass
class Plan:
    """Score columns and selections of one calibration.  With quantile levels: one RESID column per level, selected at
    the level itself, then one CQR column per interval, selected at 1 - alpha.  Without (a mean model): one ABS column
    of the metric column, selected at 1 - alpha."""
    Q: int
    levels: tuple
    intervals: tuple              # ((lo_col, hi_col), ...)
    alpha: float
    cols: list = field(default_factory=list)
    sels: list = field(default_factory=list)      # (score column, None, beta)


def make_plan(Q, levels=None, intervals=None, alpha=0.1):
    Q, alpha = int(Q), float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"conformal: alpha={alpha} must lie in (0, 1)")
    if levels is None:
        if intervals:
            raise ValueError("conformal: an interval needs quantile levels")
        plan = Plan(Q, (), (), alpha)
        plan.cols = [(ABS, Q // 2, 0)]
        plan.sels = [(0, None, interval_beta(alpha))]
        return plan
    levels = tuple(float(v) for v in levels)
    if len(levels) != Q:
        raise ValueError(f"conformal: {Q} quantile levels expected, got {len(levels)}")
    pairs = []
    for iv in (intervals or ()):
        if len(iv) != 2 or any(float(v) not in levels for v in iv):
            raise ValueError(f"conformal: interval {tuple(iv)} must name two of the quantile levels {levels}")
        lo, hi = levels.index(float(iv[0])), levels.index(float(iv[1]))
        if lo >= hi:
            raise ValueError(f"conformal: interval {tuple(iv)} must be (lower level, upper level)")
        pairs.append((lo, hi))
    if Q + len(pairs) > MAX_COLS:
        raise ValueError(f"conformal: {Q} levels and {len(pairs)} intervals are more than {MAX_COLS} score columns")
    plan = Plan(Q, levels, tuple(pairs), alpha)
    plan.cols = [(RESID, q, 0) for q in range(Q)] + [(CQR, lo, hi) for lo, hi in pairs]
    plan.sels = [(q, None, level_beta(levels[q])) for q in range(Q)] + \
                [(Q + i, None, interval_beta(alpha)) for i in range(len(pairs))]
    return plan


def finish_host(plan, segments):
    """The selections of `plan` on the calibration segment segments[0] (C, n_cal) and, with an evaluation segment
    segments[1], what the offsets do there.  Returns the dict finish_device returns."""
    cal = segments[0]
    picks = [select_level_numpy(cal[col], beta) for col, _, beta in plan.sels]
    fin = {"value": np.array([v for v, _ in picks], dtype=np.float32),
           "rank_used": np.array([r for _, r in picks], dtype=np.int64),
           "count": np.array([s.shape[1] for s in segments], dtype=np.int64),
           "overflow": np.zeros(len(segments), dtype=np.int64)}
    if len(segments) > 1:
        ev = segments[1]
        fin["before"] = np.array([(ev[col] <= 0).sum() for col, _, _ in plan.sels], dtype=np.int64)
        fin["after"] = np.array([(ev[col] <= v).sum() for (col, _, _), v in zip(plan.sels, fin["value"])], dtype=np.int64)
        fin["sums"] = ev.astype(np.float64).sum(axis=1)
    return fin


def finish_device(plan, scores, count, overflow, scratch):
    """ONE stdadk_select_f32 call on the calibration segment scores[0] (n = count[0], on the device) for every
    selection of `plan`; with an evaluation segment scores[1], per selection the count of its scores <= 0 and <= the
    offset, and per column the float64 sum of its scores; then everything is read by the host ONCE.  scores
    (G, C, cap) float32, count (G,) int64, overflow (G,) int32; scratch(name, shape, dtype) hands out the buffers."""
    from . import _native as N
    k, G, cap = len(plan.sels), scores.shape[0], scores.shape[2]
    value, rank_used = scratch("cf_value", (k,), torch.float32), scratch("cf_rank", (k,), torch.int64)
    ws = scratch("cf_select_ws", (N.select_workspace_bytes(k) // 8,), torch.float64)
    N.select(scores[0], count[0:1], plan.sels, value, rank_used, ws)
    parts = [value.double(), rank_used.double(), count.double(), overflow.double()]
    if G > 1:
        ev = scores[1]
        live = torch.arange(cap, device=scores.device) < count[1]
        e = ev[torch.tensor([s[0] for s in plan.sels], device=scores.device)]
        parts += [((e <= 0) & live).sum(dim=1).double(), ((e <= value[:, None]) & live).sum(dim=1).double(),
                  torch.where(live, ev.double(), torch.zeros((), dtype=torch.float64, device=scores.device)).sum(dim=1)]
    host = torch.cat(parts).cpu().numpy()                              # the ONE host read
    C = scores.shape[1]
    cuts = np.cumsum([k, k, G, G] + ([k, k, C] if G > 1 else []))[:-1]
    got = np.split(host, cuts)
    fin = {"value": got[0].astype(np.float32), "rank_used": got[1].astype(np.int64), "count": got[2].astype(np.int64),
           "overflow": got[3].astype(np.int64)}
    if G > 1:
        fin["before"], fin["after"], fin["sums"] = got[4].astype(np.int64), got[5].astype(np.int64), got[6]
    return fin


# ---- the record ---------------------------------------------------------------------------------------------------

@dataclass
class Calibration:
    """What a calibration found, as plain data.  `levels` (Q,) and `level_offsets` (Q,) float32: the one-sided offset of
    every quantile column (empty for a mean model); `intervals` (I, 2) the levels and `interval_cols` (I, 2) the columns
    of every interval with its CQR offset `interval_offsets` (I,) float32; `abs_offset` the half-width of a mean model
    (NaN otherwise); `n_cal` the calibration scores; `rank_used` the 0-based rank of every offset in the order levels,
    intervals (or the one ABS offset), -1 = rank beyond n_cal, offset +inf; `alpha`; `split` the calibration split.
    The guarantee is marginal over data exchangeable with that split: see the module's caveat."""
    levels: np.ndarray
    level_offsets: np.ndarray
    intervals: np.ndarray
    interval_cols: np.ndarray
    interval_offsets: np.ndarray
    abs_offset: float
    n_cal: int
    rank_used: np.ndarray
    alpha: float
    split: str = "valid"

    def apply(self, pred, interval=None):
        """Calibrated predictions from pred (..., Q), torch or numpy, in pred's own precision.  interval=None: every
        quantile column plus its one-sided offset; a mean model gives (..., 2), yhat - c and yhat + c.
        interval=(lo_level, hi_level), one of the calibrated intervals: pred with that interval widened by its CQR
        offset (q_lo - c, q_hi + c), the other columns as they are."""
        is_t = torch.is_tensor(pred)
        if interval is None and len(self.levels) == 0:
            c = float(self.abs_offset)
            col = pred[..., pred.shape[-1] // 2]
            return torch.stack([col - c, col + c], dim=-1) if is_t else np.stack([col - c, col + c], axis=-1)
        if interval is None:
            off = self.level_offsets.astype(np.float32)
            return pred + (torch.from_numpy(off).to(pred.device, pred.dtype) if is_t else off.astype(pred.dtype))
        want = (float(interval[0]), float(interval[1]))
        for (a, b), (lo, hi), c in zip(self.intervals, self.interval_cols, self.interval_offsets):
            if (float(a), float(b)) == want:
                out = pred.clone() if is_t else np.array(pred, copy=True)
                c = float(c) if is_t else out.dtype.type(c)
                out[..., int(lo)] = pred[..., int(lo)] - c
                out[..., int(hi)] = pred[..., int(hi)] + c
                return out
        raise ValueError(f"Calibration.apply: interval {want} was not calibrated (have {self.intervals.tolist()})")


def make_calibration(plan, fin, split="valid"):
    Q, I = len(plan.levels), len(plan.intervals)
    v = np.asarray(fin["value"], dtype=np.float32)
    return Calibration(levels=np.asarray(plan.levels, dtype=np.float64), level_offsets=v[:Q].copy(),
                       intervals=np.array([[plan.levels[lo], plan.levels[hi]] for lo, hi in plan.intervals],
                                          dtype=np.float64).reshape(I, 2),
                       interval_cols=np.asarray(plan.intervals, dtype=np.int64).reshape(I, 2),
                       interval_offsets=v[Q:Q + I].copy(), abs_offset=float(v[0]) if Q == 0 else float("nan"),
                       n_cal=int(fin["count"][0]), rank_used=np.asarray(fin["rank_used"], dtype=np.int64).copy(),
                       alpha=float(plan.alpha), split=str(split))


_NPZ = ("levels", "level_offsets", "intervals", "interval_cols", "interval_offsets", "abs_offset", "n_cal", "rank_used",
        "alpha", "split")


def save_calibration_npz(output_dir, cal):
    """Writes `<output_dir>/calibration.npz` and returns its path."""
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(str(output_dir), "calibration.npz")
    np.savez(path, **{k: np.asarray(getattr(cal, k)) for k in _NPZ})
    return path


def load_calibration_npz(path):
    with np.load(path) as f:
        d = {k: f[k] for k in _NPZ}
    return Calibration(levels=d["levels"], level_offsets=d["level_offsets"], intervals=d["intervals"],
                       interval_cols=d["interval_cols"], interval_offsets=d["interval_offsets"],
                       abs_offset=float(d["abs_offset"]), n_cal=int(d["n_cal"]), rank_used=d["rank_used"],
                       alpha=float(d["alpha"]), split=str(d["split"]))


def _frac(num, den):
    return float(num) / float(den) if den > 0 else float("nan")


def report(plan, fin, split="valid"):
    """The `conformal` entry of grid_scores / the dict of Predictor.conformal_grid from the host arrays of finish_*:
      alpha, split, n_cal, n_eval, overflow (per segment), rank_beyond_n (any offset +inf), calibration (the record)
      levels     {levels, offset, rank_used, reliability_before, reliability_after} (Q,) each: the one-sided offsets
                 and the share of evaluation entries with z <= q, z <= q + offset          (quantile models)
      intervals  [{interval, offset, rank_used, n_cal, coverage_before, coverage_after, mean_width_before,
                   mean_width_after}]: coverage after = #(eval scores <= offset) / n_eval, width after = before + 2 c
      abs        {half_width, rank_used, coverage}                                        (mean models)
    Evaluation figures are NaN without an evaluation segment or with an empty one."""
    Q, I = len(plan.levels), len(plan.intervals)
    ev = "after" in fin
    n_cal, n_ev = int(fin["count"][0]), int(fin["count"][1]) if ev else 0
    value, used = fin["value"], fin["rank_used"]
    share = lambda key, j: _frac(fin[key][j], n_ev) if ev else float("nan")      # noqa: E731
    out = {"alpha": plan.alpha, "split": split, "n_cal": n_cal, "n_eval": n_ev,
           "overflow": [bool(v) for v in fin["overflow"]], "rank_beyond_n": bool((used < 0).any()),
           "calibration": make_calibration(plan, fin, split)}
    if Q == 0:
        out["abs"] = {"half_width": float(value[0]), "rank_used": int(used[0]), "coverage": share("after", 0)}
        return out
    out["levels"] = {"levels": np.asarray(plan.levels, dtype=np.float64), "offset": value[:Q].copy(),
                     "rank_used": used[:Q].copy(),
                     "reliability_before": np.array([share("before", q) for q in range(Q)]),
                     "reliability_after": np.array([share("after", q) for q in range(Q)])}
    out["intervals"] = []
    for i, (lo, hi) in enumerate(plan.intervals):
        j = Q + i
        # the RESID columns of the two levels: mean(z - q_lo) - mean(z - q_hi) = the mean width
        width = _frac(fin["sums"][lo] - fin["sums"][hi], n_ev) if ev else float("nan")
        out["intervals"].append({"interval": (plan.levels[lo], plan.levels[hi]), "offset": float(value[j]),
                                 "rank_used": int(used[j]), "n_cal": n_cal, "coverage_before": share("before", j),
                                 "coverage_after": share("after", j), "mean_width_before": width,
                                 "mean_width_after": width + 2.0 * float(value[j])})
    return out


# ---- rows instead of a grid: a validation set --------------------------------------------------------------------

@torch.no_grad()
def calibrate_rows(pred, y, levels=None, intervals=None, alpha=0.1, split="valid", scratch=None):
    """A Calibration from the predictions pred (N, Q) of a calibration set and its targets y (N,): on the device (pred a
    tensor there) the set is passed to stdadk_conformal_scores_f32 as a 1 x N grid without split codes and selected by
    stdadk_select_f32, one host read; on the host the numpy restatements.  Non-finite targets are no members."""
    plan = make_plan(pred.shape[-1], levels, intervals, alpha)
    if torch.is_tensor(pred) and (pred.is_cuda or _dry_run()):
        from . import _native as N
        n = pred.shape[0]
        cache = {}
        if scratch is None:
            scratch = lambda name, shape, dtype: cache.setdefault(                       # noqa: E731
                name, torch.empty(shape, device=pred.device, dtype=dtype))
        pred = pred.contiguous().float()
        z = y.reshape(1, n).contiguous().float()
        scores = scratch("cf_scores", (1, len(plan.cols), max(n, 1)), torch.float32)
        count = scratch("cf_count", (1,), torch.int64).zero_()
        overflow = scratch("cf_overflow", (1,), torch.int32).zero_()
        if n:
            ws = scratch("cf_ws", (N.conformal_scores_workspace_bytes(n, 1) // 8,), torch.float64)
            N.conformal_scores(pred, z, None, plan.cols, [0], scores, count, overflow, ws)
        fin = finish_device(plan, scores, count, overflow, scratch)
    else:
        p = pred.detach().cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
        t = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        fin = finish_host(plan, scores_numpy(p.astype(np.float32), t.reshape(-1).astype(np.float32), None, plan.cols, [0]))
    return make_calibration(plan, fin, split)


def _dry_run():
    from . import _native as N
    return N.dry_run()
