"""`train_model` / `evaluate_model`: the reference's epoch driver (scripts/train_st_interp.py:463-881, 884-961) on
`TrainStep.run_epoch` + `Evaluator`, over device-resident `DeviceDataset`s.

Per epoch: progressive unfreezing of the knot group (:582-602), one pass of optimisation steps with the manual
warm-up (:715-720: the first step runs at the full rate, the factor applies from the second), validation under the EMA
weights (:737-806), the cosine schedule (:524-530,820-822; a real CosineAnnealingLR on a two-group dummy optimiser
whose rates are fed to `set_lr` / `set_basis_lr`, so its `eta_min = lr/2` for the knot group and its interplay with
the manual rate changes are the reference's, not a restatement), best state / patience / early stop (:829-857).
Host syncs per epoch: one read for the training loss, one for validation.

`train_loss` is the reference's mean of BATCH means (`TrainStep.run_epoch(loss="batches")`: a 4-byte device copy of
the accumulator before the last, ragged batch gives both partial sums with the epoch's one read).

The best state is a copy of the EMA buffer on the device; `model_best.pt` (the reference's `state_dict` keys, EMA
values) and `training_history.csv` are written once, at the end, when `output_dir` is given.

`checkpoint=path` saves the engine's state and the driver's own (schedule, best state, patience, history, permutation
RNG) at epoch ends (`stnf.checkpoint`); `resume=True` continues from that file as the same run: parameters, moments,
shadow and every history column but `train_loss` (a float-atomic sum) are the bits the uninterrupted run has."""
import csv
import json
import math
import os
import warnings

import torch

from .checkpoint import read_checkpoint, save_checkpoint
from .engine import TrainStep
from .evaluation import Evaluator
from .flat import _bump_engine_version


def loss_settings(model, config):
    """(loss kind, quantile levels, non-crossing weight, power, lambda) from the reference's config keys."""
    rt = config.get("regression_type", "mean")
    if rt == "mean":
        return "mse", None, 0.0, 1, 0.0
    if rt == "quantile":
        q = config.get("current_quantile", None)
        if q is None:
            raise ValueError("current_quantile must be specified for quantile regression")
        return "pinball", [float(q)], 0.0, 1, 0.0
    if rt == "multi-quantile":
        levels = [float(q) for q in config.get("quantile_levels", [0.1, 0.5, 0.9])]
        if config.get("use_delta_reparameterization", False):
            return "pinball", levels, 0.0, 1, float(config.get("non_crossing_lambda", 0.0))
        return "pinball", levels, float(config.get("non_crossing_weight", 0.0)), \
            int(config.get("non_crossing_power", 1)), 0.0
    raise ValueError(f"Unknown regression_type: {rt}")


def make_evaluator(model, config, max_batch=65536):
    kind, levels, ncw, ncp, ncl = loss_settings(model, config)
    return Evaluator(model, loss=kind, quantile_levels=levels, non_crossing_weight=ncw, non_crossing_power=ncp,
                     non_crossing_lambda=ncl, max_batch=max_batch)


def val_batch_size(batch_size, n):
    """scripts/train_st_interp.py:2292-2293"""
    return max(1, min(max(int(batch_size) * 16, 32768), int(n)))


def evaluate_model(model, data, config=None):
    """The reference's metric dict (`mse, mae, rmse` [+ `check_loss`, `mean_check_loss`, `crps`]) of the model's
    current parameters on a `DeviceDataset`, plus `loss` (mean batch objective); one host sync.  With
    `quantile_diagnostics: true` in the config a quantile model's dict gains `quantile` (Evaluator.evaluate)."""
    config = config or {}
    bs = int(config.get("val_batch_size", 0)) or val_batch_size(config.get("batch_size", 256), len(data))
    out = make_evaluator(model, config, max_batch=bs).evaluate(
        data, bs, diagnostics=config.get("quantile_diagnostics", False))
    out.pop("rows", None)
    return out


class _Schedule:
    """The learning rates of the reference's two parameter groups, kept by the real torch scheduler."""

    def __init__(self, config, learnable):
        self.lr = float(config.get("lr", 1e-3))
        self.unfreeze = int(config.get("basis_unfreeze_epoch", 0)) if learnable else 0
        self.rampup = int(config.get("basis_lr_rampup_epochs", 0))
        target = self.lr * float(config.get("basis_lr_ratio", 0.05))
        groups = [{"params": [torch.zeros(1, requires_grad=True)], "lr": self.lr, "name": "mlp"}]
        if learnable:
            groups.append({"params": [torch.zeros(1, requires_grad=True)],
                           "lr": 0.0 if self.unfreeze > 0 else target, "name": "basis"})
        self.opt = torch.optim.SGD(groups, lr=self.lr)
        for g in self.opt.param_groups:
            g["initial_lr"] = g["lr"]
            if g["name"] == "basis":
                g["target_lr"] = target
        self.sched = None
        if config.get("scheduler") == "cosine":
            self.sched = torch.optim.lr_scheduler.CosineAnnealingLR(self.opt, T_max=config.get("epochs", 100),
                                                                    eta_min=self.lr * 0.5)
        self.warmup_epochs = int(config.get("warmup_epochs", 0))
        self.warmup_steps = 0
        self.global_step = 0

    @property
    def groups(self):
        return self.opt.param_groups

    def start_epoch(self, epoch):
        """Progressive unfreezing, scripts/train_st_interp.py:582-602."""
        if self.unfreeze <= 0 or len(self.groups) < 2:
            return
        g = self.groups[1]
        if epoch == self.unfreeze:
            g["lr"] = g["target_lr"] * 0.1 if self.rampup > 0 else g["target_lr"]
        elif self.unfreeze < epoch < self.unfreeze + self.rampup:
            g["lr"] = g["target_lr"] * (0.1 + 0.9 * (epoch - self.unfreeze) / self.rampup)

    def after_step(self):
        """Manual warm-up, :715-720 (runs after the optimiser step: it sets the NEXT step's rate)."""
        if self.global_step < self.warmup_steps:
            f = (self.global_step + 1) / self.warmup_steps
            for g in self.groups:
                g["lr"] = g["initial_lr"] * f
        self.global_step += 1

    def end_epoch(self, epoch):
        """:820-822"""
        if self.sched is not None and epoch >= self.warmup_epochs:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")        # (the dummy optimiser never steps)
                self.sched.step()


def make_engine(model, config, batch_size, batches_per_epoch):
    """TrainStep with the reference driver's settings (config keys and code defaults of :463-541,660-707)."""
    kind, levels, ncw, ncp, ncl = loss_settings(model, config)
    return TrainStep(model, lr=float(config.get("lr", 1e-3)), weight_decay=float(config.get("weight_decay", 1e-5)),
                     grad_clip=float(config.get("grad_clip", 0) or 0.0),
                     ema_decay=1.0 - 1.0 / (10.0 * batches_per_epoch), max_batch=int(batch_size),
                     loss=kind, quantile_levels=levels, non_crossing_weight=ncw, non_crossing_power=ncp,
                     non_crossing_lambda=ncl, basis_lr_ratio=float(config.get("basis_lr_ratio", 0.05)),
                     domain_penalty_weight=float(config.get("domain_penalty_weight", 0.0)),
                     movement_penalty_weight=float(config.get("movement_penalty_weight", 0.0)),
                     sparsity_penalty_type=config.get("sparsity_penalty_type", "none"),
                     sparsity_lambda_l1=config.get("sparsity_lambda_l1", 0.001),
                     sparsity_lambda_group=config.get("sparsity_lambda_group", 0.01),
                     sparsity_apply_to_spatial=config.get("sparsity_apply_to_spatial", True),
                     sparsity_apply_to_temporal=config.get("sparsity_apply_to_temporal", True),
                     seed=config.get("dropout_seed", None), dtype=config.get("dtype", "f32"),
                     fused_knot_step=config.get("fused_knot_step", None),
                     fused_delta_step=config.get("fused_delta_step", None))


def _ema_full(eng):
    """The whole EMA shadow as one flat tensor (a view of `eng.ema`, or gathered when the optimiser is sharded)."""
    if not eng.shard:
        return eng.ema
    eng.swap_in_ema()
    full = eng.flat.clone()
    eng.swap_in_ema()
    return full


def _load_flat(eng, flat_values):
    """Overwrite the live parameters with `flat_values` (flat layout); derived copies follow."""
    eng.flat.copy_(flat_values)
    _bump_engine_version(eng.model)
    eng.refresh_bf16()


_NOT_COMPARED = ("verbose", "checkpoint", "checkpoint_every", "resume")     # config keys a resumed run may change


def _json_items(config):
    """The items of `config` that JSON can write, each as its JSON text (tuples and lists, 1 and 1.0 compare as the
    reference's YAML would read them back)."""
    out = {}
    for k, v in config.items():
        try:
            out[str(k)] = json.dumps(v, sort_keys=True)
        except (TypeError, ValueError):
            pass
    return out


def _rng_state(generator, dev):
    """State of whatever draws the epoch permutations: the caller's generator, else torch's default generators (the
    device's draws randperm; the host's is kept with it).  Reads only."""
    if generator is not None:
        return {"generator": generator.get_state()}
    out = {"cpu": torch.get_rng_state()}
    if dev.type == "cuda":
        out["device"] = torch.cuda.get_rng_state(dev)
    return out


def _set_rng_state(state, generator, dev):
    if generator is not None:
        generator.set_state(state["generator"])
        return
    torch.set_rng_state(state["cpu"])
    if dev.type == "cuda" and "device" in state:
        torch.cuda.set_rng_state(state["device"], dev)


def train_model(model, train_data, val_data, config, device=None, output_dir=None, generator=None, shuffle=True,
                engine=None, evaluator=None, checkpoint=None, checkpoint_every=1, resume=False):
    """scripts/train_st_interp.py:463-881 on device-resident data.  Returns (model, history, basis_centers_history);
    the model ends up holding the best EMA state (or the final EMA state when no epoch was ever best).
    `engine` / `evaluator`: ready-made TrainStep (`make_engine`) / Evaluator-like object, for callers who want to keep
    the engine (its `best_ema` attribute is the device-side best state afterwards, None when no epoch was best) or
    bring their own settings.  Single process: data-parallel training drives TrainStep.run_epoch / Evaluator itself.

    Non-finite training loss: the reference leaves the epoch at the first NaN batch (:724-733), after that batch's
    optimiser step has already made the parameters NaN.  Here the epoch runs through by default (no host sync per
    step) and ends in the same state: NaN parameters and shadow, NaN `train_loss`, a validation loss that is never
    best.  `config["nan_check_every"] = k` polls the device guard every k steps and leaves the epoch there.

    `checkpoint` (a path): the run is saved there at the end of every `checkpoint_every`-th epoch and of the last one,
    after the best / patience update and the scheduler step (`stnf.checkpoint.save_checkpoint`: the engine's state plus
    the driver's; the previous file survives an interrupted write).  `resume=True` continues from that file when it
    exists -- on a fresh model and engine of the same configuration, the same data and the same kind of `generator` --
    at the saved epoch; a file of a run that had already stopped goes straight to the final state without a step.  A
    config key that differs (other than `verbose`) is a ValueError naming it.  Epoch ends only: a run killed inside an
    epoch repeats that epoch."""
    if device is not None:
        model.to(device)
    learnable = bool(config.get("spatial_learnable", False)) and bool(model.spatial_basis.learnable)
    batch_size = int(config.get("batch_size", 256))
    n_batches = max(1, math.ceil(len(train_data) / batch_size))
    model.train()
    eng = engine if engine is not None else make_engine(model, config, batch_size, n_batches)
    vbs = int(config.get("val_batch_size", 0)) or val_batch_size(batch_size, len(val_data))
    ev = evaluator if evaluator is not None else make_evaluator(model, config, max_batch=vbs)
    verbose = bool(config.get("verbose", True))

    sch = _Schedule(config, learnable)
    sch.warmup_steps = sch.warmup_epochs * n_batches if sch.warmup_epochs > 0 else 0
    epochs = int(config.get("epochs", 100))
    patience = int(config.get("patience", 15))
    check_every = int(config.get("nan_check_every", 0))
    best_val, patience_counter = float("inf"), 0
    best_state, has_best = torch.empty_like(eng.flat), False
    history = {"train_loss": [], "val_loss": [], "val_rmse": [], "lr": []}
    centers_history = []
    applied = {}

    def on_step(i, batches):
        # this step's rates (device scalars: a fill each, and only when a rate changed), then the warm-up's next
        groups = sch.groups
        if applied.get("lr") != groups[0]["lr"]:
            eng.set_lr(groups[0]["lr"])
            applied["lr"] = groups[0]["lr"]
        if learnable and applied.get("basis") != groups[1]["lr"]:
            eng.set_basis_lr(groups[1]["lr"])
            applied["basis"] = groups[1]["lr"]
        sch.after_step()

    def driver_state(next_epoch, stopped):
        """The driver's half of a checkpoint (tensors on the host, numbers, strings, lists, dicts)."""
        return {"epoch": next_epoch, "stopped": bool(stopped), "rows": len(train_data), "shuffle": bool(shuffle),
                "groups": [{k: g[k] for k in ("lr", "initial_lr", "target_lr") if k in g} for g in sch.groups],
                "sched": sch.sched.state_dict() if sch.sched is not None else None,
                "global_step": sch.global_step, "warmup_steps": sch.warmup_steps,
                "best_val": best_val, "patience_counter": patience_counter, "has_best": has_best,
                "best_state": best_state.cpu() if has_best else None,
                "history": {k: list(v) for k, v in history.items()},
                "centers_history": [[e, torch.from_numpy(c)] for e, c in centers_history],
                "applied": dict(applied), "rng": _rng_state(generator, eng.dev), "config": _json_items(config)}

    first_epoch = 0
    if resume and checkpoint is None:
        raise ValueError("checkpoint: resume=True needs the path of the checkpoint")
    if resume and os.path.exists(str(checkpoint)):
        ck = read_checkpoint(checkpoint)
        saved = ck["extra"]
        theirs, ours = saved["config"], _json_items(config)
        for k in sorted(set(theirs) | set(ours)):
            if k not in _NOT_COMPARED and theirs.get(k) != ours.get(k):
                raise ValueError(f"config['{k}']: the checkpoint was written with {theirs.get(k)}, this call has "
                                 f"{ours.get(k)}")
        for k, own in (("rows", len(train_data)), ("shuffle", bool(shuffle))):
            if saved[k] != own:
                raise ValueError(f"{k}: the checkpoint was written with {saved[k]}, this call has {own}")
        if (generator is not None) != ("generator" in saved["rng"]):
            raise ValueError("generator: the checkpoint was written " + ("with" if "generator" in saved["rng"] else "without")
                             + " a permutation generator, this call is " + ("with" if generator is not None else "without")
                             + " one")
        eng.load_state_dict(ck["engine"])              # (every refusal above and in here comes before the first write)
        _set_rng_state(saved["rng"], generator, eng.dev)
        if verbose:
            print(f"Resuming from {checkpoint}: " + ("the run had stopped" if saved["stopped"]
                                                     else f"epoch {saved['epoch'] + 1}/{epochs}"), flush=True)
        for g, fields in zip(sch.groups, saved["groups"]):
            g.update(fields)
        if sch.sched is not None:
            sch.sched.load_state_dict(saved["sched"])
        sch.global_step, sch.warmup_steps = saved["global_step"], saved["warmup_steps"]
        best_val, patience_counter, has_best = saved["best_val"], saved["patience_counter"], saved["has_best"]
        if has_best:
            best_state.copy_(saved["best_state"])
        history = {k: list(v) for k, v in saved["history"].items()}
        centers_history = [(e, c.numpy().copy()) for e, c in saved["centers_history"]]
        applied.update(saved["applied"])
        first_epoch = epochs if saved["stopped"] else saved["epoch"]

    for epoch in range(first_epoch, epochs):
        sch.start_epoch(epoch)
        model.train()
        # the reference's train_loss: mean of batch means, one read (TrainStep.run_epoch, loss="batches")
        train_loss = eng.run_epoch(train_data, batch_size, generator=generator, shuffle=shuffle, check_every=check_every,
                                   on_step=on_step, loss="batches")

        model.eval()
        val = ev.evaluate(val_data, vbs, params="ema", engine=eng)
        val_loss, val_rmse = float(val["loss"]), float(val["rmse"])
        history["train_loss"].append(train_loss)
        history["val_loss"].append(val_loss)
        history["val_rmse"].append(val_rmse)
        current_lr = sch.groups[0]["lr"]
        history["lr"].append(current_lr)                 # (recorded before the scheduler steps, as the reference does)
        line = f"Epoch {epoch + 1}/{epochs}: Train={train_loss:.6f}, Val={val_loss:.6f}, RMSE={val_rmse:.6f}"
        sch.end_epoch(epoch)
        if sch.sched is not None and epoch >= sch.warmup_epochs:
            line += f", LR={sch.sched.get_last_lr()[0]:.6f}"
        elif epoch < sch.warmup_epochs:
            line += f", LR={current_lr:.6f}(warmup)"
        if not math.isnan(val_loss) and val_loss < best_val:
            best_val, patience_counter, has_best = val_loss, 0, True
            best_state.copy_(_ema_full(eng))             # on the device; written out once, at the end
            line += " [Best]"
        else:
            patience_counter += 1
            line += f" ({patience_counter}/{patience})"
        if verbose:
            print(line, flush=True)
        if learnable and (epoch + 1) % 100 == 0:
            centers_history.append((epoch + 1, model.spatial_basis.centers.detach().cpu().numpy().copy()))
        stopping = patience_counter >= patience or epoch + 1 == epochs
        if checkpoint is not None and (stopping or (epoch + 1) % max(int(checkpoint_every), 1) == 0):
            save_checkpoint(checkpoint, eng, driver_state(epoch + 1, stopping))
        if patience_counter >= patience:
            if verbose:
                print(f"\nEarly stopping triggered at epoch {epoch + 1}")
            break

    # the best EMA state (or the final EMA state) becomes the model, :860-866
    _load_flat(eng, best_state if has_best else _ema_full(eng))
    eng.best_ema = best_state if has_best else None     # the device-side copy the model was loaded from
    model.eval()
    if output_dir is not None:
        os.makedirs(str(output_dir), exist_ok=True)
        if has_best:
            torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                       os.path.join(str(output_dir), "model_best.pt"))
        with open(os.path.join(str(output_dir), "training_history.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["epoch", "train_loss", "val_loss", "val_rmse", "lr"])
            for i in range(len(history["train_loss"])):
                w.writerow([i + 1] + [repr(float(history[k][i])) for k in ("train_loss", "val_loss", "val_rmse", "lr")])
    return model, history, centers_history
