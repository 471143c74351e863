"""Cases of the train_model golden (make_training_golden.py writes it where the reference is on disk; the tests read it
anywhere).  Numpy-only and deterministic, like cases.py: inputs and initial weights are rebuilt from seeds on both
sides, the .npz files hold the reference's recorded histories and learning rates only."""
try:
    from . import cases
except ImportError:        # run next to the generator (tests/golden on sys.path)
    import cases

TRAIN_ROWS, VAL_ROWS, BATCH = 1000, 700, 300          # 300 + 300 + 300 + 100 training, 300 + 300 + 100 validation

_COMMON = dict(lr=2e-2, epochs=3, batch_size=BATCH, warmup_epochs=1, scheduler="cosine", grad_clip=10.0, patience=15)

# (a) fixed knots + MSE; (b) the shipped shape: learnable knots + 5 quantiles + non-crossing weight, knots unfrozen at
# epoch 1 with a 2-epoch ramp (so all of warm-up, unfreezing and the cosine recursion act within 3 epochs)
TRAIN_CASES = {
    "train_fixed_mse": dict(base="default227", seed=61, output_dim=1, learnable=False,
                            config=dict(_COMMON, regression_type="mean")),
    "train_learn_mq5": dict(base="default227", seed=62, output_dim=5, learnable=True,
                            knots=dict(gradient_damping=True, damping_threshold=0.0, damping_strength=5.0),
                            config=dict(_COMMON, regression_type="multi-quantile", quantile_levels=cases.TAUS5,
                                        non_crossing_weight=0.5, non_crossing_power=1, spatial_learnable=True,
                                        basis_lr_ratio=0.05, domain_penalty_weight=0.01, basis_unfreeze_epoch=1,
                                        basis_lr_rampup_epochs=2)),
}

# schedule-only runs of the reference's train_model on a tiny model (8 epochs, 200 rows in batches of 64): the learning
# rate of every parameter group at every optimiser step and the history's lr column
SCHED_ROWS, SCHED_VAL_ROWS, SCHED_BATCH = 200, 150, 64
_SCHED = dict(lr=2e-2, epochs=8, batch_size=SCHED_BATCH, warmup_epochs=1, scheduler="cosine", grad_clip=10.0,
              patience=100, regression_type="mean")
SCHED_CASES = {
    "sched_fixed": dict(base="tiny9", seed=71, output_dim=1, learnable=False, config=dict(_SCHED)),
    "sched_learn": dict(base="tiny9", seed=72, output_dim=1, learnable=True, knots={},
                        config=dict(_SCHED, spatial_learnable=True, basis_unfreeze_epoch=2, basis_lr_rampup_epochs=2)),
    "sched_learn_now": dict(base="tiny9", seed=73, output_dim=1, learnable=True, knots={},
                            config=dict(_SCHED, spatial_learnable=True, warmup_epochs=2)),
}


def model_cfg(case):
    cfg = dict(cases.MODEL_CASES[case["base"]])
    cfg.update(seed=case["seed"], output_dim=case["output_dim"])
    return cfg


def data(case, rows, val_rows):
    """(X, coords, t, y) float32 arrays of the training and the validation set."""
    cfg = model_cfg(case)
    return (cases.make_inputs(dict(cfg, B=rows)), cases.make_inputs(dict(cfg, B=val_rows, seed=cfg["seed"] + 500)))
