"""A resumed run is the same run: TrainStep.state_dict / load_state_dict and train_model(checkpoint=, resume=) on the
device, bit for bit.

Engine level: 1 000 rows in batches of 300 (the last of an epoch has 100 rows), dropout 0.1, clipping on, a rate that
changes every step, `step_indexed` with the `next_idx` announcements `run_epoch` makes.  5 steps, a file, a fresh
model and engine with another initialisation and another dropout seed, 4 more steps -- the cut falls between a step
that pre-binned its successor and a step that starts cold -- against 9 uninterrupted steps.  The same into an engine
that has already stepped under its own seed (an announced batch, inline or on the side stream; captured graphs).
Driver level: both tests/golden/training_cases.TRAIN_CASES configurations with dropout 0.1, shuffled by a device
generator, 4 epochs, killed in the third epoch's validation and resumed by a fresh model and engine.

Yardstick: a second uninterrupted run (at engine level the run that took the state_dict, which also shows that saving
perturbs nothing).  Whatever the two uninterrupted runs agree on bitwise -- expected of parameters, moments, shadow,
step counter, guard word and the lr / val_loss / val_rmse columns -- the resumed run must agree on bitwise.  The float-
atomic loss accumulator (mean_loss(), the train_loss column) is the one exception: 1e-6 relative, the margin
tests/test_gpu_round3.py uses for it.  Every comparison is printed."""
import math
import os

import numpy as np
import pytest
import torch

from golden import cases
from golden import training_cases as tc
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

ROWS, BATCH, STEPS, CUT = 1000, 300, 9, 5
LOSS_RTOL = 1e-6

# name -> (model shape, window route expected, model settings, engine settings)
_KNOTS = dict(spatial_learnable=True, gradient_damping=True, damping_threshold=0.0, damping_strength=5.0)
_PENALTIES = dict(domain_penalty_weight=0.01, movement_penalty_weight=0.05)
_MQ5 = dict(loss="pinball", quantile_levels=cases.TAUS5)
# P_nc(delta) <= 0 is summed into the same float accumulator as the (positive) check loss.  A float32 sum is accurate
# relative to the sum of MAGNITUDES, so the relative margin on mean_loss() means what it says only while the two do not
# cancel: at lambda = 0.05 the penalty outweighed the check loss over these nine steps (mean objective -0.21) and two
# uninterrupted runs already differed by 5e-7 relative; lambda = 0.005 keeps the penalty a fraction of the data term (mean
# objective +0.43, uninterrupted runs within 2e-7).  (The state comparisons are bitwise at either lambda.)
_NC_LAMBDA = 0.005
ENGINE_CASES = {
    "fixed_window_f32": ("c2_b257", True, {}, {}),
    "fixed_window_bf16": ("c2_b257", True, {}, dict(dtype="bf16")),
    "fixed_window_graph": ("c2_b257", True, {}, dict(use_graph=True)),
    "fixed_window_side_stream": ("c2_b257", True, {}, dict(inline_prep=False)),
    "fixed_materialising": ("default227", False, {}, {}),
    "learn_split": ("default227", False, _KNOTS, dict(_PENALTIES, fused_knot_step=False)),
    "learn_fused_window": ("c2_b257", True, _KNOTS, dict(_PENALTIES, fused_knot_step=True)),
    "delta_learn_fused": ("c2_b257", True, dict(_KNOTS, output_dim=5, use_delta_reparameterization=True),
                          dict(_PENALTIES, **_MQ5, non_crossing_lambda=_NC_LAMBDA, fused_delta_step=True)),
    "delta_learn_split": ("default227", False, dict(_KNOTS, output_dim=5, use_delta_reparameterization=True),
                          dict(_PENALTIES, **_MQ5, non_crossing_lambda=_NC_LAMBDA, fused_delta_step=False,
                               fused_knot_step=False)),
    "sparse_group": ("c2_b257", True, {}, dict(sparsity_penalty_type="sparse_group", sparsity_lambda_l1=1e-4,
                                               sparsity_lambda_group=1e-3)),
}


def _model(base, init_seed, **kw):
    """The case's shape with dropout 0.1 and torch's own initialisation under `init_seed`; learnable knots start off
    their grid (cases.knot_perturbation), so that damping and the movement penalty act."""
    from stnf.models import STInterpMLP
    cfg = cases.MODEL_CASES[base]
    torch.manual_seed(init_seed)
    m = STInterpMLP(p=0, k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=cfg["k_temporal_centers"],
                    hidden_dims=cfg["hidden_dims"], dropout=0.1, layernorm=True, **kw)
    if kw.get("spatial_learnable"):
        dc, dlb = cases.knot_perturbation(cfg)
        with torch.no_grad():
            m.spatial_basis.centers += torch.from_numpy(dc) * (1 + init_seed)
            m.spatial_basis.log_bandwidths += torch.from_numpy(dlb)
    m.train()
    return m.to(dev())


def _engine(name, init_seed, dropout_seed):
    from stnf.engine import TrainStep
    base, window, mkw, ekw = ENGINE_CASES[name]
    eng = TrainStep(_model(base, init_seed, **mkw), lr=2e-2, weight_decay=5e-4, grad_clip=10.0, ema_decay=0.99,
                    max_batch=BATCH, seed=dropout_seed, **ekw)
    assert eng.uses_window == window, (name, eng.uses_window)
    # the door the case is named after (the environment could otherwise switch a default to a one-call step)
    door = "knots" if ekw.get("fused_knot_step") else "delta" if ekw.get("fused_delta_step") else "split" if mkw else "whole"
    assert (eng._whole_step, eng._knot_step, eng._delta_step) == (door == "whole", door == "knots", door == "delta"), name
    return eng


@pytest.fixture(scope="module")
def observations():
    _, coords, t, y = (torch.from_numpy(a).to(dev()) for a in cases.make_inputs(dict(cases.MODEL_CASES["c2_b257"], B=ROWS)))
    g = torch.Generator().manual_seed(123)
    plan = []                   # (idx, next_idx) per step, as run_epoch announces: nothing after an epoch's last batch
    while len(plan) < STEPS:
        batches = torch.randperm(ROWS, generator=g).to(dev()).split(BATCH)
        plan += [(b, batches[i + 1] if i + 1 < len(batches) else None) for i, b in enumerate(batches)]
    assert plan[CUT - 1][1] is not None and plan[CUT - 1][0].numel() == BATCH and plan[3][0].numel() == ROWS % BATCH
    return coords, t, y, plan[:STEPS]


def _steps(eng, observations, first, last):
    coords, t, y, plan = observations
    for i in range(first, last):
        eng.set_lr(2e-2 * (1.0 - 0.05 * i))
        if eng.learnable:
            eng.set_basis_lr(1e-3 * (1.0 - 0.05 * i))
        idx, nxt = plan[i]
        eng.step_indexed(coords, t, y, idx, next_idx=nxt)


def _bits(eng):
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).clone() for k in ("flat", "m", "v", "ema", "step_dev", "nonfinite")}
    out.update({"buffer " + n: b.clone() for n, b in eng.model.named_buffers()})
    return out


def _judge(what, control, control2, resumed):
    """`resumed` against `control` wherever `control2` (a second uninterrupted run) agrees with it bitwise; the two
    controls are expected to agree everywhere."""
    controls_differ = []
    for k in control:
        same = torch.equal(control[k], control2[k])
        got = torch.equal(resumed[k], control[k])
        print(f"{what} {k}: uninterrupted runs agree {same}, resumed equals uninterrupted {got}"
              + ("" if got else f" ({int((resumed[k] != control[k]).sum())} of {control[k].numel()} differ)"))
        if not same:
            controls_differ.append(k)
        else:
            assert got, (what, k)
    assert not controls_differ, f"{what}: two uninterrupted runs differ in {controls_differ} (not a checkpoint matter)"


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_resumed_steps_are_the_uninterrupted_steps(name, observations, tmp_path):
    from stnf.checkpoint import load_checkpoint, save_checkpoint
    whole = _engine(name, 0, 5)
    if name == "fixed_window_f32":
        assert whole._pack_table is not None             # the packed fp32 weight copies are rebuilt by the load
    _steps(whole, observations, 0, STEPS)
    want = _bits(whole)
    loss_whole = whole.mean_loss()
    del whole

    saver = _engine(name, 0, 5)
    _steps(saver, observations, 0, CUT)
    # on the window route (eager chain) step 5 has announced step 6's batch: the saving run starts step 6 on it
    assert (saver._prepared is not None) == (saver.uses_window and not saver.use_graph)
    path = os.path.join(tmp_path, "engine.pt")
    save_checkpoint(path, saver, extra={"step": CUT})
    _steps(saver, observations, CUT, STEPS)                         # the saving run goes on: the second control
    control2 = _bits(saver)
    loss_saver = saver.mean_loss()
    del saver

    fresh = _engine(name, 1, 99)
    assert not torch.equal(fresh.flat, want["flat"])
    addresses = [t.data_ptr() for t in (fresh.flat, fresh.m, fresh.v, fresh.ema, fresh.step_dev)]
    assert load_checkpoint(path, fresh) == {"step": CUT}
    assert addresses == [t.data_ptr() for t in (fresh.flat, fresh.m, fresh.v, fresh.ema, fresh.step_dev)]
    assert fresh.step_count == CUT and int(fresh.step_dev.item()) == CUT and fresh.base_seed == 5
    _steps(fresh, observations, CUT, STEPS)
    got = _bits(fresh)
    loss_resumed = fresh.mean_loss()

    assert int(want["step_dev"].item()) == STEPS and int(want["nonfinite"].item()) == 0
    _judge(name, want, control2, got)
    for what, value in (("saving run", loss_saver), ("resumed run", loss_resumed)):
        rel = abs(value - loss_whole) / abs(loss_whole)
        print(f"{name} mean_loss over {STEPS} steps: uninterrupted {loss_whole:.9g}, {what} {value:.9g}, relative {rel:.3g}")
        assert math.isfinite(loss_whole) and rel <= LOSS_RTOL, (what, value, loss_whole)


@pytest.mark.parametrize("name", ["fixed_window_f32", "fixed_window_side_stream", "fixed_window_graph"])
def test_load_into_an_engine_that_has_stepped(name, observations, tmp_path):
    """The loading engine is not fresh: it has taken 3 steps of its own under another dropout seed, so it holds an
    announced batch (binned inside its last step, or still being binned on the side stream) or chains captured with ITS
    seed by value.  After the load its next 4 steps are the uninterrupted run's."""
    from stnf.checkpoint import load_checkpoint, save_checkpoint
    whole = _engine(name, 0, 5)
    _steps(whole, observations, 0, CUT)
    path = os.path.join(tmp_path, "engine.pt")
    save_checkpoint(path, whole)
    _steps(whole, observations, CUT, STEPS)
    want = _bits(whole)
    del whole

    used = _engine(name, 1, 99)
    _steps(used, observations, 0, 3)
    if used.use_graph:
        assert not used._ix_graph.stale(used._ix_graph.key)
    else:
        assert used._prepared is not None and used._prepared.inline == (name == "fixed_window_f32")
    load_checkpoint(path, used)
    assert used._prepared is None and used._ix_graph.stale(used._ix_graph.key) and used._graph.stale(used._graph.key)
    _steps(used, observations, CUT, STEPS)
    got = _bits(used)
    for k in want:
        same = torch.equal(got[k], want[k])
        print(f"{name} {k}: loaded into a used engine, equals uninterrupted {same}")
        assert same, (name, k)


# ------------------------------------------------------------------------------------------------ train_model
class Killed(Exception):
    pass


HANDICAP = 1000.0


class _Scripted:
    """The real evaluator, `first` epochs into the run.  `alive`: after that many calls the next one is where the
    process 'dies'.  `handicap_from`: from that epoch (1-based) on HANDICAP is added to the validation loss, so that no
    later epoch is best and the final best state can only be an earlier one."""

    def __init__(self, ev, alive=None, first=0, handicap_from=None):
        self.ev, self.alive, self.first, self.handicap_from, self.calls = ev, alive, first, handicap_from, 0

    def evaluate(self, *a, **kw):
        self.calls += 1
        if self.alive is not None and self.calls > self.alive:
            raise Killed()
        out = self.ev.evaluate(*a, **kw)
        if self.handicap_from is not None and self.first + self.calls >= self.handicap_from:
            out = dict(out, loss=out["loss"] + HANDICAP)
        return out


def _driver_run(case, data, config, seed, out_dir, alive=None, first=0, handicap_from=None, **kw):
    """One train_model call on a fresh model and engine: initialisation, dropout base seed and the permutation
    generator's starting point all follow `seed`."""
    from stnf import training as T
    from stnf.models import STInterpMLP
    cfg = tc.model_cfg(case)
    kn = case.get("knots", {})
    torch.manual_seed(seed)
    m = STInterpMLP(p=cfg["p"], k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=cfg["k_temporal_centers"],
                    hidden_dims=cfg["hidden_dims"], dropout=0.1, layernorm=cfg["layernorm"],
                    spatial_learnable=case["learnable"], spatial_basis_function=cfg["basis"], output_dim=cfg["output_dim"],
                    gradient_damping=kn.get("gradient_damping", False), damping_threshold=kn.get("damping_threshold", 0.3),
                    damping_strength=kn.get("damping_strength", 1.0)).to(dev())
    eng = T.make_engine(m, config, tc.BATCH, math.ceil(tc.TRAIN_ROWS / tc.BATCH))       # (base seed: torch's generator)
    ev = T.make_evaluator(m, config, max_batch=tc.BATCH)
    gen = torch.Generator(device=dev()).manual_seed(1000 + seed)
    try:
        model, hist, _ = T.train_model(m, data[0], data[1], config, output_dir=out_dir, generator=gen, shuffle=True,
                                       engine=eng, evaluator=_Scripted(ev, alive, first, handicap_from), **kw)
    except Killed:
        torch.cuda.synchronize()
        return None
    torch.cuda.synchronize()
    return {"hist": hist, "model": {k: v.detach().clone() for k, v in model.state_dict().items()},
            "best_ema": eng.best_ema.clone(), "file": torch.load(os.path.join(out_dir, "model_best.pt")),
            "steps": eng.step_count}


@pytest.mark.parametrize("best", ["as_it_falls", "before_the_cut"])
@pytest.mark.parametrize("name", list(tc.TRAIN_CASES))
def test_resumed_training_is_the_uninterrupted_training(name, best, tmp_path):
    """Runs A (checkpointing on), A0 (off), B (dies in the third validation), C (a fresh model and engine, resumed).
    `before_the_cut`: the validation losses of epochs 3 and 4 carry a handicap, so the best epoch lies before the cut
    and the resumed run's best value, patience counter and best state -- the model it returns, model_best.pt -- can
    only be the file's."""
    from test_gpu_training_golden import _dataset
    case = tc.TRAIN_CASES[name]
    cfg = tc.model_cfg(case)
    tr, va = tc.data(case, tc.TRAIN_ROWS, tc.VAL_ROWS)
    data = (_dataset(tr, cfg["p"]), _dataset(va, cfg["p"]))
    config = dict(case["config"], epochs=4, val_batch_size=tc.BATCH, verbose=False)
    ck = os.path.join(tmp_path, "run.pt")
    hc = dict(handicap_from=3 if best == "before_the_cut" else None)
    a = _driver_run(case, data, config, 0, os.path.join(tmp_path, "a"), checkpoint=os.path.join(tmp_path, "a.pt"), **hc)
    a0 = _driver_run(case, data, config, 0, os.path.join(tmp_path, "a0"), **hc)
    assert _driver_run(case, data, config, 0, os.path.join(tmp_path, "b"), alive=2, checkpoint=ck, **hc) is None
    saved = torch.load(ck, map_location="cpu", weights_only=True)["extra"]
    assert saved["epoch"] == 2 and not saved["stopped"] and saved["has_best"]
    assert saved["best_val"] == min(a["hist"]["val_loss"][:2])
    assert saved["patience_counter"] == (0 if a["hist"]["val_loss"][1] < a["hist"]["val_loss"][0] else 1)
    c = _driver_run(case, data, config, 1, os.path.join(tmp_path, "c"), first=2, checkpoint=ck, resume=True, **hc)
    if best == "before_the_cut":
        assert min(a["hist"]["val_loss"][2:]) > HANDICAP > min(a["hist"]["val_loss"][:2])
        assert torch.equal(saved["best_state"].to(dev()), a["best_ema"])           # the file's tensor IS the final best
    assert a["steps"] == a0["steps"] == c["steps"] == 4 * math.ceil(tc.TRAIN_ROWS / tc.BATCH)

    def flat(run):
        out = {"hist " + col: torch.tensor(run["hist"][col], dtype=torch.float64) for col in ("lr", "val_loss", "val_rmse")}
        out.update({"model " + k: v for k, v in run["model"].items()})
        out.update({"model_best.pt " + k: v.to(dev()) for k, v in run["file"].items()})
        out["best_ema"] = run["best_ema"]
        return out
    assert all(np.isfinite(a["hist"][col]).all() for col in a["hist"])
    _judge(f"{name} {best}", flat(a), flat(a0), flat(c))
    for e in range(4):
        for what, run in (("checkpointing off", a0), ("resumed", c)):
            x, y = a["hist"]["train_loss"][e], run["hist"]["train_loss"][e]
            rel = abs(x - y) / abs(x)
            print(f"{name} train_loss[{e}]: uninterrupted {x:.9g}, {what} {y:.9g}, relative {rel:.3g}")
            assert rel <= LOSS_RTOL, (what, e, x, y)
