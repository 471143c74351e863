"""On-device validation: `Evaluator` runs the reference's evaluation passes (scripts/train_st_interp.py:737-806,
884-961) over a `DeviceDataset` through stdadk_eval_indexed_f32 -- an indexed, forward-only pass per batch whose
metric sums stay in a float64 accumulator on the device.  One host sync per call (one read of the accumulator).

EMA weights (`params="ema"`, with the `TrainStep` that owns the shadow):
  * fixed knots, no delta head, replicated optimiser -- the north-star path and every BASELINE configuration: the
    parameter table points INTO `engine.ema` (same flat layout as the live buffer, W0 stored transposed), so nothing is
    copied and nothing is swapped.  In bf16 mode the pass keeps the bf16 matrix cores: operand copies of the EMA
    values are rounded into buffers of the evaluator's own by one stdadk_bf16_shadow_refresh launch per call;
  * learnable knots, the delta head, the sharded optimiser: the pass is bracketed by `engine.swap_in_ema()`.
Either way the live parameters, Adam moments, the shadow and the step counter are the same bits afterwards."""
import torch
import torch.distributed as dist

from . import _native as N
from . import losses


class Evaluator:
    """evaluate(dataset, batch_size, params="live"|"ema", engine=None) -> dict with the reference's keys
    `mse, mae, rmse` (of the median level `Q // 2` for several outputs), `check_loss` (quantile), `mean_check_loss`,
    `check_loss`, `crps` (multi-quantile), plus `loss`: the mean over batches of the batch objective, the
    reference's `val_loss` (with the delta head and `non_crossing_lambda > 0` the parameter-level P_nc(delta) is part
    of every batch's objective, as scripts/train_st_interp.py:770-777 has it).  `batch_size` is one size (last batch
    ragged) or a list of sizes summing to len(dataset), the data-parallel schedule of `DeviceDataset.epoch_batches`.
    `diagnostics=True` (pinball objectives; ignored without quantile levels): the batches keep their predictions in one
    (N, Q) buffer in dataset order (`self.predictions` afterwards), one stdadk_quantile_diag_f32 call reduces it against
    the targets into a second accumulator -- all-reduced and read in the same host sync as the first -- and the dict
    gains `quantile`: levels, reliability, pit, cross_rate, pair_cross_rate, nc_penalty_p1, nc_penalty_p2, crps, rows
    (stnf.utils.predictions.quantile_diagnostics; `self.quantile_sums` holds the sums)."""

    def __init__(self, model, loss="mse", quantile_levels=None, non_crossing_weight=0.0, non_crossing_power=1,
                 non_crossing_lambda=0.0, max_batch=65536, force_dense=False, process_group=None):
        self.model = model
        self.objective = losses.Objective(model, loss, quantile_levels, non_crossing_weight, non_crossing_power,
                                          non_crossing_lambda)
        self.max_batch = int(max_batch)
        self.force_dense = bool(force_dense)
        self.pg = process_group
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda" and not N.dry_run():
            raise RuntimeError("Evaluator needs the model on a HIP device; there is no CPU path")
        self.acc = torch.zeros(N.EVAL_SLOTS, dtype=torch.float64, device=self.dev)
        self.sums = None               # the accumulator of the last call as host floats
        self.quantile_sums = None      # diagnostics=True: the QD_SLOTS sums of the last call as host floats
        self.predictions = None        # diagnostics=True: the (N, Q) predictions of the last call, dataset order
        self._desc = None
        self._ws = {}
        self._ema = None               # (key, parameter table over engine.ema, bf16 refresh table or None)

    # ------------------------------------------------------------------------------------
    def _loss_desc(self, y_cols):
        return self.objective.desc(y_cols)

    def _workspace(self, basis, desc, B, flags):
        B = max(int(B), self.max_batch)
        key = int(flags)
        ws = self._ws.get(key)
        need = N.eval_workspace_bytes(basis, desc, B, flags)
        if ws is None or ws.numel() * 4 < need:
            ws = self._ws[key] = torch.empty((need + 3) // 4, device=self.dev)
        return ws

    @staticmethod
    def ema_in_place(engine):
        """True when the EMA pass reads `engine.ema` through views (no swap): fixed knots, no delta head,
        replicated optimiser."""
        return not engine.learnable and not engine.model._has_delta and not engine.shard

    def _ema_params(self, eng):
        """Parameter table over views of `eng.ema` (the flat layout of `eng.flat`: first weight stored (in,out))."""
        m = self.model
        key = (eng.ema.data_ptr(), eng.flat.data_ptr(), eng.dtype)
        if self._ema is not None and self._ema[0] == key:
            return self._ema[1], self._ema[2]
        lay = eng.layout
        tensors = [lay.view(eng.ema, p) for p in m._body_params()]
        pairs, table = None, None
        if eng._shadow_regions:
            # bf16 mode: operand copies of the EMA values in buffers of our own, re-rounded at the start of every pass
            pairs, regions = lay.hidden_copies(
                lambda h, hp: (torch.empty(h, hp, device=self.dev, dtype=torch.bfloat16),
                               torch.empty(hp, h, device=self.dev, dtype=torch.bfloat16)))
            table = N.make_bf16_shadow(regions)
        params = m._pack(tensors, bf16=pairs)
        params._views = (tensors, pairs)          # the descriptors hold raw addresses: keep the tensors alive
        self._ema = (key, params, table)
        return params, table

    # ------------------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate(self, dataset, batch_size, params="live", engine=None, diagnostics=False, conformal=None,
                 conformal_interval=None):
        """`conformal=alpha` (off by default): `dataset` is the CALIBRATION split; the batches keep their predictions as
        with `diagnostics` and the dict gains `calibration`, a stnf.calibration.Calibration at miscoverage alpha made
        from them on the device (stdadk_conformal_scores_f32 on the set as a 1 x N grid, stdadk_select_f32; one more
        host read): for a pinball objective a one-sided offset per level and the CQR offset of `conformal_interval`
        (two of the levels; default the outermost two), otherwise the half-width of |y - yhat|.  The guarantee is
        marginal over data exchangeable with this set: with site-wise splits, new sites drawn like the validation
        sites, not every site.  Single process only."""
        if params not in ("live", "ema"):
            raise ValueError(f"params='{params}'; use 'live' or 'ema'")
        m = self.model
        swapped = False
        if params == "ema":
            if engine is None or engine.ema is None:
                raise RuntimeError("params='ema' needs the TrainStep that owns the shadow (built with ema_decay)")
            if engine.model is not m:
                raise RuntimeError("the engine trains another model")
            if not self.ema_in_place(engine):
                engine.swap_in_ema()
                swapped = True
        try:
            # (a list of sizes summing to len(dataset): the data-parallel schedule, DeviceDataset.epoch_batches)
            sizes = [int(b) for b in batch_size] if isinstance(batch_size, (list, tuple)) else int(batch_size)
            out = self._evaluate(dataset, sizes, engine, ema_views=(params == "ema" and not swapped),
                                 diagnostics=bool(diagnostics) and self.objective.kind == "pinball",
                                 keep=conformal is not None)
            if conformal is not None:
                out["calibration"] = self._calibrate(dataset, float(conformal), conformal_interval)
            return out
        finally:
            if swapped:
                engine.swap_in_ema()

    def _calibrate(self, dataset, alpha, interval):
        """The Calibration of the pass that just ran, from the predictions it kept (dataset order)."""
        from .calibration import calibrate_rows
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1:
            raise NotImplementedError("Evaluator: conformal calibration runs in a single process (the order statistic "
                                      "of a sharded set is not a sum over ranks)")
        levels = self.objective.quantile_levels if self.objective.kind == "pinball" else None
        if levels is not None and interval is None and len(levels) >= 2:
            interval = (levels[0], levels[-1])
        y = dataset.y
        target = y.view(-1) if y.shape[1] == 1 else y[:, self.model.output_dim // 2].contiguous()
        return calibrate_rows(self.predictions, target, levels, [interval] if interval is not None else None, alpha,
                              scratch=self._buffer)

    def _evaluate(self, dataset, batch_size, engine, ema_views, diagnostics=False, keep=False):
        m = self.model
        if self._desc is None:
            self._desc = m._native_desc(False)
        desc = self._desc
        if engine is not None:
            engine._check_bf16_current()
            st = engine.state
            basis, flags, ptab = st.basis, st.flags, st.params
            if self.force_dense:
                flags |= N.FLAG_DENSE
            if st.head is not None:
                N.delta_head(st.delta, st.head[0], st.head[1])     # output layer of the delta values as they are now
            if ema_views:
                ptab, table = self._ema_params(engine)
                if table is not None:
                    N.bf16_shadow_refresh(engine.ema, table)
        else:
            st = m._step_state(self.dev, force_dense=self.force_dense, training=False)
            basis, flags, ptab = st.basis, st.flags, st.params
        Q = m.output_dim
        metric_col = Q // 2
        y_all = dataset.y
        ldesc = self._loss_desc(y_all.shape[1])
        X_all = dataset.X if m.p > 0 else None
        t_all = dataset.t.view(-1)
        batches = dataset.epoch_batches(batch_size, shuffle=False) if len(dataset) else ()
        ws = self._workspace(basis, desc, max((b.numel() for b in batches), default=1), flags)
        acc = self.acc
        acc.zero_()
        n_rows = len(dataset)
        preds = self._buffer("preds", (n_rows, Q), torch.float32) if diagnostics or keep else None
        if keep:
            self.predictions = preds
        row = 0
        for idx in batches:
            B = idx.numel()
            N.eval_indexed(basis, desc, ptab, dataset.coords, t_all, X_all, y_all,
                           N._contig(idx), ldesc, metric_col, 1.0 / (B * Q), acc,
                           None if preds is None else preds[row:row + B], ws, flags)
            row += B
        if self.objective.nc_lambda > 0.0 and len(batches):
            # parameter-level penalty of the delta head: the same value in every batch's objective
            p_nc = losses.compute_p_nc_delta_penalty(list(m.delta_params))
            acc[N.EVAL_OBJECTIVE] += (self.objective.nc_lambda * len(batches)) * p_nc.double()
        accs = [acc]
        if diagnostics:
            # the set as a 1 x N "grid" without splits: no site or time sums (the batches are consecutive slices of
            # the set, so the buffer is in dataset order and the targets are read where they are)
            qacc = self._buffer("qacc", (4, N.QD_SLOTS), torch.float64).zero_()
            if n_rows:
                target = y_all if y_all.shape[1] == 1 else y_all[:, metric_col].contiguous()
                qws = self._buffer("qws", (N.quantile_diag_workspace_bytes(n_rows, 1) // 8,), torch.float64)
                N.quantile_diag(preds, target.view(1, n_rows), None, self.objective.quantile_levels, -1, -1, qacc,
                                None, None, qws)
            accs.append(qacc[0])
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1:
            for a in accs:
                dist.all_reduce(a, op=dist.ReduceOp.SUM, group=self.pg)
        host = (torch.cat(accs) if diagnostics else acc).tolist()  # the call's ONE host sync
        self.sums = host[:N.EVAL_SLOTS]
        out = self.metrics(self.sums)
        if diagnostics:
            import numpy as np
            from .utils.predictions import quantile_diagnostics
            self.quantile_sums, self.predictions = host[N.EVAL_SLOTS:], preds
            sums = np.zeros((4, N.QD_SLOTS))
            sums[0] = self.quantile_sums
            out["quantile"] = quantile_diagnostics(sums, None, None, self.objective.quantile_levels, False)["all"]
        return out

    def _buffer(self, name, shape, dtype):
        """Scratch of the diagnostics, kept between calls."""
        buf = self._ws.get(name)
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype:
            buf = self._ws[name] = torch.empty(shape, device=self.dev, dtype=dtype)
        return buf

    def metrics(self, sums):
        """The reference's metric dict from the accumulator's sums."""
        Q = self.model.output_dim
        rows, nb = max(sums[N.EVAL_ROWS], 1.0), max(sums[N.EVAL_BATCHES], 1.0)
        mse = sums[N.EVAL_SSE] / rows
        out = {"mse": mse, "mae": sums[N.EVAL_SAE] / rows, "rmse": mse ** 0.5,
               "loss": sums[N.EVAL_OBJECTIVE] / nb, "rows": int(sums[N.EVAL_ROWS])}
        if self.objective.kind == "pinball":
            checks = [sums[N.EVAL_CHECK + q] / rows for q in range(Q)]
            if Q == 1:
                out["check_loss"] = checks[0]
            else:
                # compute_crps_multi_quantile with its default weights: 2 x sum_k (1/K) x check loss at level k
                out["crps"] = 2.0 * sum(c / Q for c in checks)
                out["mean_check_loss"] = sum(checks) / Q
                out["check_loss"] = out["mean_check_loss"]
        return out
