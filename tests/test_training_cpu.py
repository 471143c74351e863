"""CPU tests of stnf.training / stnf.evaluation / stdadk_eval_indexed_f32 (no GPU): with STDADK_DRY_RUN=1 the library
validates and plans but launches nothing, so the epoch driver's control flow, its learning-rate sequence and the
library calls of a validated epoch can be checked on host tensors.  stnf._native reads the variable at import, so this
file is its own driver: run as a script in a child process it prints one JSON record, which the tests read."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, EPOCHS, BATCH, ROWS, VAL_ROWS = 2e-2, 8, 64, 200, 150


def _record(tmp):
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    import torch
    from stnf import _native as N
    from stnf import training as T
    from stnf.dataio.device_dataset import DeviceDataset
    from stnf.engine import TrainStep
    from stnf.evaluation import Evaluator
    from stnf.models import STInterpMLP

    def model(**kw):
        torch.manual_seed(0)
        return STInterpMLP(p=0, k_spatial_centers=[25, 81], k_temporal_centers=[10, 15], hidden_dims=[64, 64],
                           dropout=0.0, layernorm=True, **kw)

    def data(n, seed):
        g = torch.Generator().manual_seed(seed)
        return DeviceDataset(torch.rand(n, 2, generator=g), torch.rand(n, 1, generator=g), torch.randn(n, 1, generator=g))

    class Stub:
        """Scripted validation losses; records what it was asked."""
        def __init__(self, losses):
            self.losses, self.calls = list(losses), []

        def evaluate(self, dataset, batch_size, params="live", engine=None):
            self.calls.append((len(dataset), batch_size, params))
            v = self.losses[len(self.calls) - 1]
            return {"loss": v, "rmse": abs(v) ** 0.5 if v == v else v, "mse": v, "mae": v}

    def watch(eng, log):
        for name in ("set_lr", "set_basis_lr"):
            fn = getattr(eng, name)
            setattr(eng, name, (lambda f, n: lambda v: (log.append([n, eng.step_count, float(v)]), f(v))[1])(fn, name))

    rec = {}
    # --- 1. schedule + control flow: fixed knots, warm-up 1 epoch, cosine, scripted validation
    cfg = {"lr": LR, "epochs": EPOCHS, "batch_size": BATCH, "warmup_epochs": 1, "scheduler": "cosine", "patience": 3,
           "grad_clip": 10.0, "verbose": False}
    losses = [0.9, 0.5, float("nan"), 0.7, 0.4, 0.45, 0.41, 0.6]
    m = model()
    n_batches = math.ceil(ROWS / BATCH)
    eng = T.make_engine(m, cfg, BATCH, n_batches)
    log = []
    watch(eng, log)
    stub = Stub(losses)
    out_dir = os.path.join(tmp, "run1")
    _, hist, _ = T.train_model(m, data(ROWS, 1), data(VAL_ROWS, 2), cfg, output_dir=out_dir, shuffle=False, engine=eng,
                               evaluator=stub)
    rec["fixed"] = {"hist": hist, "rates": log, "stub_calls": stub.calls, "files": sorted(os.listdir(out_dir)),
                    "steps": eng.step_count, "ema_decay": eng.ema_decay, "wd": eng.wd,
                    "csv": open(os.path.join(out_dir, "training_history.csv")).read().splitlines(),
                    "keys": sorted(torch.load(os.path.join(out_dir, "model_best.pt")).keys()),
                    "model_keys": sorted(m.state_dict().keys())}
    # --- early stop + every validation NaN: no best, final EMA loaded, no model_best.pt
    cfg2 = dict(cfg, patience=2, warmup_epochs=0)
    m = model()
    eng = T.make_engine(m, cfg2, BATCH, n_batches)
    stub = Stub([float("nan")] * EPOCHS)
    out_dir = os.path.join(tmp, "run2")
    _, hist, _ = T.train_model(m, data(ROWS, 1), data(VAL_ROWS, 2), cfg2, output_dir=out_dir, shuffle=False, engine=eng,
                               evaluator=stub)
    rec["nan"] = {"epochs": len(hist["val_loss"]), "files": sorted(os.listdir(out_dir)),
                  "best": eng.best_ema is None}
    # --- the reference's schedules (tests/golden/sched_*.npz): the rate of every group at every step
    from golden import training_cases as tc
    rec["sched"] = {}
    for name, case in tc.SCHED_CASES.items():
        c = dict(case["config"], verbose=False)
        m = model(spatial_learnable=True) if case["learnable"] else model()
        nb = math.ceil(tc.SCHED_ROWS / tc.SCHED_BATCH)
        eng = T.make_engine(m, c, tc.SCHED_BATCH, nb)
        cur = {"set_lr": None, "set_basis_lr": None}
        per_step = []
        for nm in cur:
            fn = getattr(eng, nm)
            setattr(eng, nm, (lambda f, n: lambda v: (cur.__setitem__(n, float(v)), f(v))[1])(fn, nm))
        step = eng.step_indexed

        def stepping(*a, _step=step, _cur=cur, _out=per_step, _learn=case["learnable"], **kw):
            _out.append([_cur["set_lr"]] + ([_cur["set_basis_lr"]] if _learn else []))
            return _step(*a, **kw)
        eng.step_indexed = stepping
        _, hist, _ = T.train_model(m, data(tc.SCHED_ROWS, 1), data(tc.SCHED_VAL_ROWS, 2), c, shuffle=False, engine=eng,
                                   evaluator=Stub([1.0 / (i + 1) for i in range(c["epochs"])]))
        rec["sched"][name] = {"rates": per_step, "lr": hist["lr"]}

    # --- 2. call trace of one validated epoch
    real = N.lib()
    calls = []

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name in ("stdadk_last_error", "stdadk_abi_version"):
                return fn

            def call(*args):
                calls.append((name, args))
                return fn(*args)
            return call
    N.lib = lambda: Proxy()

    def scalars(name, args):
        types = N._SIGNATURES[name][1]
        out = [name]
        for t, a in zip(types, args):
            if t in (C.c_int64, C.c_int32, C.c_size_t):
                out.append(int(a))
            elif t in (C.c_float, C.c_double):
                out.append(float(a))
        return out

    def is_eval(name):
        return name.startswith("stdadk_eval_")

    def trace_plain():
        m = model()
        cfgt = {"lr": LR, "batch_size": BATCH, "grad_clip": 10.0}
        eng = T.make_engine(m, cfgt, BATCH, n_batches)
        del calls[:]
        eng.run_epoch(data(ROWS, 1), BATCH, shuffle=False)
        return [scalars(n, a) for n, a in calls]

    def trace_driver(warmup):
        """One epoch as train_model runs it (on_step rates, loss="batches", validation under EMA)."""
        m = model()
        cfgt = {"lr": LR, "batch_size": BATCH, "grad_clip": 10.0, "epochs": 1, "warmup_epochs": warmup,
                "scheduler": "cosine", "val_batch_size": BATCH, "verbose": False}
        eng = T.make_engine(m, cfgt, BATCH, n_batches)
        lo, hi = eng.ema.data_ptr(), eng.ema.data_ptr() + eng.ema.numel() * 4
        copies = []
        clone, copy_ = torch.Tensor.clone, torch.Tensor.copy_
        big = eng.flat.numel()

        def counting_clone(t, *a, **kw):
            if t.numel() >= big:
                copies.append("clone")
            return clone(t, *a, **kw)

        def counting_copy(t, src, *a, **kw):
            if t.numel() >= big:
                copies.append("copy_")
            return copy_(t, src, *a, **kw)
        del calls[:]
        torch.Tensor.clone, torch.Tensor.copy_ = counting_clone, counting_copy
        try:
            T.train_model(m, data(ROWS, 1), data(VAL_ROWS, 2), cfgt, shuffle=False, engine=eng)
        finally:
            torch.Tensor.clone, torch.Tensor.copy_ = clone, copy_
        inside = []
        for n, a in calls:
            if n == "stdadk_eval_indexed_f32":
                tab = a[2]._obj
                ptrs = [p for arr in (tab.W, tab.b, tab.ln_g, tab.ln_b) for p in arr if p]
                inside.append(all(lo <= p < hi for p in ptrs) and len(ptrs) > 0)
        return {"train": [scalars(n, a) for n, a in calls if not is_eval(n)],
                "eval": [scalars(n, a) for n, a in calls if is_eval(n)], "inside_ema": inside,
                # one epoch, it is the best: ONE copy of the shadow into the best state, one load of it at the end
                "flat_copies": copies, "ema_in_place": Evaluator.ema_in_place(eng)}
    rec["trace_plain"] = trace_plain()
    rec["trace_driver"] = {str(w): trace_driver(w) for w in (0, 1)}

    # --- 3. argument errors of the new entry
    m = model()
    eng = TrainStep(m, max_batch=BATCH, ema_decay=0.99, seed=1)
    ev = Evaluator(m, max_batch=BATCH)
    va = data(VAL_ROWS, 2)
    st = eng.state
    desc = m._native_desc(False)
    ws = torch.empty(N.eval_workspace_bytes(st.basis, desc, BATCH, st.flags) // 4)
    acc = torch.zeros(N.EVAL_SLOTS, dtype=torch.float64)
    idx = torch.arange(BATCH)

    def attempt(**kw):
        a = dict(basis=st.basis, desc=desc, params=st.params, coords_all=va.coords, t_all=va.t.view(-1), X_all=None,
                 y_all=va.y, idx=idx, loss_desc=None, metric_col=0, batch_weight=1.0 / BATCH, acc=acc, y_pred=None,
                 workspace=ws, flags=st.flags)
        a.update(kw)
        try:
            N.eval_indexed(**a)
            return "ok"
        except RuntimeError as e:
            return str(e)
    rec["errors"] = {"ok": attempt(), "null_coords": attempt(coords_all=None), "null_y": attempt(y_all=None),
                     "big_B": attempt(idx=torch.arange(4 * BATCH)), "metric_col": attempt(metric_col=1),
                     "metric_neg": attempt(metric_col=-1), "small_ws": attempt(workspace=ws[:ws.numel() // 2])}
    null_acc = real.stdadk_eval_indexed_f32(C.byref(st.basis), C.byref(desc), C.byref(st.params), va.coords.data_ptr(),
                                            va.t.data_ptr(), None, va.y.data_ptr(), idx.data_ptr(), BATCH, None, 0,
                                            1.0 / BATCH, None, None, ws.data_ptr(), ws.numel() * 4, st.flags, None)
    rec["errors"]["null_acc"] = [null_acc, real.stdadk_last_error().decode()]

    # --- 4. refusals of the optimiser entry points: code and text
    def refused(fn, *a, **kw):
        try:
            fn(*a, **kw)
            return "ok"
        except RuntimeError as e:
            return str(e)
    n = 64
    p_, g_, m_, v_, e_ = (torch.zeros(n + 4) for _ in range(5))
    bufs = (p_[:n], g_[:n], m_[:n], v_[:n], e_[:n])
    parts, word, watch = torch.zeros(N.SUMSQ_PARTS), torch.zeros(1, dtype=torch.int32), torch.zeros(1)
    half = torch.zeros(32, dtype=torch.bfloat16)
    shadow = N.make_bf16_shadow([(0, 4, 8, half, None)])
    hyper = ((0.9, 0.999), 1e-8, 0.0, 1)
    group = N.make_adam_group(*bufs, 1e-3)
    rec["optim_errors"] = {
        "ok": refused(N.adamw_ema, *bufs, 1e-3, *hyper, max_norm=1.0, sumsq_parts=parts, shadow=shadow,
                      loss_watch=watch, nonfinite_step=word),
        "ok2": refused(N.adamw_ema2, group, group, *hyper, loss_watch=watch, nonfinite_step=word),
        "empty_ok": refused(N.adamw_ema, *(b[:0] for b in bufs), 1e-3, *hyper),
        "clip": refused(N.adamw_ema, *bufs, 1e-3, *hyper, max_norm=1.0),
        "clip2": refused(N.adamw_ema2, group, N.make_adam_group(*bufs, 1e-3, max_norm=1.0), *hyper),
        "watch": refused(N.adamw_ema, *bufs, 1e-3, *hyper, loss_watch=watch),
        "watch2": refused(N.adamw_ema2, group, group, *hyper, nonfinite_step=word),
        "shadow": refused(N.adamw_ema, p_[:n], g_[1:n + 1], m_[:n], v_[:n], e_[:n], 1e-3, *hyper, shadow=shadow),
        "shadow2": refused(N.adamw_ema2, group, N.make_adam_group(p_[:n], g_[:n], m_[1:n + 1], v_[:n], e_[:n], 1e-3,
                                                                 shadow=shadow), *hyper),
        "empty2": refused(N.adamw_ema2, group, N.make_adam_group(*(b[:0] for b in bufs), 1e-3), *hyper),
        "step0": refused(N.adamw_ema, *bufs, 1e-3, (0.9, 0.999), 1e-8, 0.0, 0),
    }
    eng = TrainStep(model(), max_batch=BATCH, ema_decay=0.99, seed=1)
    tr = data(BATCH, 3)

    def one_call(**kw):
        a = dict(p=eng.flat, g=eng.grad, m=eng.m, v=eng.v, ema=eng.ema, lr=1e-3, lr_dev=None, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, step_dev=eng.step_dev, max_norm=1.0, sumsq_parts=eng._sumsq512, ema_decay=0.99)
        a.update(kw)
        st = eng.state
        return refused(N.train_step, st.basis, st.desc, st.params, eng.grads_t, tr.coords, tr.t.view(-1), None, tr.y, None,
                       BATCH, 1.0 / BATCH, eng.loss_sum, eng.ws, st.flags, N.make_optim(**a))
    rec["optim_errors"].update({"desc_ok": one_call(), "desc_no_step": one_call(step_dev=None),
                                "desc_no_m": one_call(m=None), "desc_clip": one_call(sumsq_parts=None)})

    # --- 5. refusals of the step opener and the four training doors: code and text, straight from the C ABI
    DOORS = {   # argument names in ABI order
        "train_fwd_bwd": "b d P G coords t X y B grad_scale loss loss_sum y_pred ws ws_bytes seed step_dev flags stream aux",
        "train_fwd_bwd_indexed": "b d P G coords t X y idx B grad_scale loss loss_sum y_pred ws ws_bytes seed step_dev flags "
                                 "stream aux",
        "train_step": "b d P G coords t X y idx B grad_scale loss sparsity loss_sum ws ws_bytes seed flags o stream",
        "train_step_next": "b d P G coords t X y idx B grad_scale loss sparsity loss_sum ws ws_bytes seed flags o next_idx "
                           "next_B next_y_cols next_ws next_ws_bytes next_binned stream",
    }

    done = C.c_int32(7)

    def doors_of(p):
        """door(name, **changed arguments) -> [code, text] on a model with p covariates."""
        torch.manual_seed(0)    # (the window path needs a first hidden layer of 128 or 256 units)
        eng = TrainStep(STInterpMLP(p=p, k_spatial_centers=[25, 81], k_temporal_centers=[10, 15], hidden_dims=[128, 64],
                                    dropout=0.0, layernorm=True), max_batch=BATCH, ema_decay=0.99, seed=1)
        st = eng.state
        win = st.flags | N.FLAG_WINDOW
        assert N.step_uses_window(st.basis, st.desc, win) and not N.step_uses_window(st.basis, st.desc, st.flags)
        idx, nxt = torch.arange(BATCH), torch.arange(BATCH)
        ws_w = torch.empty(max(N.step_workspace_bytes(st.basis, st.desc, BATCH, f) for f in (win, st.flags)) // 4 + 4)
        ws_n = torch.empty_like(ws_w)
        no_hidden = type(st.desc)()
        C.memmove(C.byref(no_hidden), C.byref(st.desc), C.sizeof(no_hidden))
        no_hidden.n_hidden = 0
        optim = N.make_optim(p=eng.flat, g=eng.grad, m=eng.m, v=eng.v, ema=eng.ema, lr=1e-3, lr_dev=None, betas=(0.9, 0.999),
                             eps=1e-8, weight_decay=0.0, step_dev=eng.step_dev, max_norm=1.0, sumsq_parts=eng._sumsq512,
                             ema_decay=0.99)
        X = torch.randn(BATCH, max(p, 1))

        def door(name, **kw):
            a = dict(b=C.byref(st.basis), d=C.byref(st.desc), P=C.byref(st.params), G=C.byref(eng.grads_t),
                     coords=tr.coords.data_ptr(), t=tr.t.data_ptr(), X=X.data_ptr() if p else None, y=tr.y.data_ptr(),
                     idx=None, B=BATCH, grad_scale=1.0 / BATCH, loss=None, sparsity=None, loss_sum=eng.loss_sum.data_ptr(), y_pred=None,
                     ws=ws_w.data_ptr(), ws_bytes=ws_w.numel() * 4, seed=0, step_dev=eng.step_dev.data_ptr(), flags=st.flags,
                     stream=None, aux=None, o=C.byref(optim), next_idx=nxt.data_ptr(), next_B=BATCH, next_y_cols=1,
                     next_ws=ws_n.data_ptr(), next_ws_bytes=ws_n.numel() * 4, next_binned=C.byref(done))
            if name in ("train_fwd_bwd_indexed", "train_step_next"):
                a.update(idx=idx.data_ptr(), flags=win)
            a.update(kw)
            rc = getattr(real, f"stdadk_{name}_f32")(*[a[k] for k in DOORS[name].split()])
            return [rc, real.stdadk_last_error().decode() if rc else ""]
        door.idx, door.ws, door.next_ws, door.no_hidden, door.dense, door.win = idx, ws_w, ws_n, no_hidden, st.flags, win
        return door
    door = doors_of(0)
    dense, win = door.dense, door.win
    r = {}
    for name in DOORS:
        r[name + ":ok"] = door(name)
        r[name + ":null_P"] = door(name, P=None)
        r[name + ":null_G"] = door(name, G=None)
        r[name + ":null_desc"] = door(name, d=None)
        r[name + ":null_basis"] = door(name, b=None)
        r[name + ":bad_B"] = door(name, B=-1)
        r[name + ":null_ws"] = door(name, ws=None)
        r[name + ":ws_misaligned"] = door(name, ws=door.ws.data_ptr() + 4)
        r[name + ":ws_small"] = door(name, ws_bytes=256)
        r[name + ":null_coords"] = door(name, coords=None)
        r[name + ":null_y"] = door(name, y=None)
        r[name + ":bf16_no_tail"] = door(name, d=C.byref(door.no_hidden), flags=dense | N.FLAG_BF16)
        r[name + ":bad_loss"] = door(name, loss=C.byref(N.make_loss("mse", Q=1, y_cols=3)))
        # two mistakes at once: the first check in the door's order speaks
        r[name + ":ws_small+null_P"] = door(name, ws_bytes=256, P=None)
        r[name + ":null_P+bad_loss"] = door(name, P=None, loss=C.byref(N.make_loss("mse", Q=1, y_cols=3)))
    for name in ("train_fwd_bwd", "train_step"):
        r[name + ":prebinned_dense"] = door(name, flags=dense | N.FLAG_PREBINNED)
        r[name + ":prebinned_window_ok"] = door(name, flags=win | N.FLAG_PREBINNED, coords=None, y=None)
    r["train_step:idx_dense+null_P"] = door("train_step", idx=door.idx.data_ptr(), P=None)
    r["train_step:idx_dense"] = door("train_step", idx=door.idx.data_ptr())
    r["train_fwd_bwd_indexed:idx_dense"] = door("train_fwd_bwd_indexed", flags=dense)
    r["train_fwd_bwd_indexed:null_idx"] = door("train_fwd_bwd_indexed", idx=None)
    r["train_fwd_bwd_indexed:null_idx+null_P"] = door("train_fwd_bwd_indexed", idx=None, P=None)
    r["train_fwd_bwd_indexed:null_idx_B0"] = door("train_fwd_bwd_indexed", idx=None, B=0)
    r["train_step_next:null_binned"] = door("train_step_next", next_binned=None)
    r["train_step_next:null_binned+no_optim"] = door("train_step_next", next_binned=None, o=None)
    r["train_step_next:no_optim"] = door("train_step_next", o=None)
    r["train_step_next:y_cols_high"] = door("train_step_next", next_y_cols=2)
    r["train_step_next:y_cols_neg"] = door("train_step_next", next_y_cols=-1)
    r["train_step_next:y_cols_no_y"] = door("train_step_next", y=None, flags=win | N.FLAG_PREBINNED)
    r["train_step_next:next_ws_small"] = door("train_step_next", next_ws_bytes=256)
    r["train_step_next:next_ws_small+null_P"] = door("train_step_next", next_ws_bytes=256, P=None)
    r["train_step_next:next_ws_misaligned"] = door("train_step_next", next_ws=door.next_ws.data_ptr() + 4)
    r["train_step_next:next_B_bad"] = door("train_step_next", next_B=1 << 31)
    done.value = 7
    r["train_step_next:binned_flag"] = [door("train_step_next")[0], done.value]
    done.value = 7
    r["train_step_next:binned_reset_on_error"] = [door("train_step_next", P=None)[0], done.value]
    # covariates (p = 2): X is asked for after the other pointers and before the loss descriptor, unless the batch is binned
    door = doors_of(2)
    bad_loss = C.byref(N.make_loss("mse", Q=1, y_cols=3))
    for name in DOORS:
        r[name + ":p2_ok"] = door(name)
        r[name + ":p2_null_X"] = door(name, X=None)
        r[name + ":p2_null_X+bad_loss"] = door(name, X=None, loss=bad_loss)
        r[name + ":p2_null_X+null_coords"] = door(name, X=None, coords=None)
        r[name + ":p2_null_X+ws_small"] = door(name, X=None, ws_bytes=256)
        r[name + ":p2_null_X_prebinned"] = door(name, X=None, flags=door.win | N.FLAG_PREBINNED)
    rec["step_errors"] = r
    print("RECORD " + json.dumps(rec))


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("training"))
    env = dict(os.environ, STDADK_DRY_RUN="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), tmp], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RECORD ")][-1]
    return json.loads(line[len("RECORD "):])


@pytest.mark.parametrize("name", ["sched_fixed", "sched_learn", "sched_learn_now"])
def test_learning_rates_equal_the_reference(rec, name):
    """Every group's rate at every optimiser step and the history's lr column against what the reference's own
    train_model used (recorded by tests/golden/make_training_golden.py): warm-up, unfreezing with its ramp, and the
    cosine recursion acting on the manually written knot rates.  Host arithmetic: equal to 1e-12."""
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    got = np.asarray(rec["sched"][name]["rates"], np.float64)
    assert got.shape == g["rates"].shape, (got.shape, g["rates"].shape)
    assert np.all(np.abs(got - g["rates"]) <= 1e-12 * np.abs(g["rates"])), np.argwhere(got != g["rates"])[:5]
    lr = np.asarray(rec["sched"][name]["lr"], np.float64)
    assert lr.shape == g["lr"].shape and np.all(np.abs(lr - g["lr"]) <= 1e-12 * np.abs(g["lr"]))


def test_driver_settings(rec):
    r = rec["fixed"]
    nb = math.ceil(ROWS / BATCH)
    assert r["ema_decay"] == pytest.approx(1.0 - 1.0 / (10.0 * nb), rel=1e-15)
    assert r["wd"] == 1e-5                      # the code default of the reference driver, not the YAML's


def test_best_patience_early_stop_and_files(rec):
    r = rec["fixed"]
    # scripted validation losses 0.9 0.5 nan 0.7 0.4 0.45 0.41 0.6, patience 3: best at epochs 1, 2, 5; the NaN never
    # becomes best; epochs 6, 7, 8 do not improve -> early stop after the 8th
    assert len(r["hist"]["val_loss"]) == 8
    assert [c[2] for c in r["stub_calls"]] == ["ema"] * 8
    assert all(c[0] == VAL_ROWS and c[1] == min(max(16 * BATCH, 32768), VAL_ROWS) for c in r["stub_calls"])
    assert r["files"] == ["model_best.pt", "training_history.csv"]
    assert r["csv"][0] == "epoch,train_loss,val_loss,val_rmse,lr" and len(r["csv"]) == 9
    assert r["keys"] == r["model_keys"]
    n = rec["nan"]
    assert n["epochs"] == 2 and n["files"] == ["training_history.csv"] and n["best"]


@pytest.mark.parametrize("warmup", ["0", "1"])
def test_call_trace_of_a_validated_epoch(rec, warmup):
    """One epoch as train_model runs it -- per-step rates, batch-mean loss, validation under EMA, best state -- makes
    the library calls of a plain run_epoch, then one stdadk_eval_indexed_f32 per validation batch on views of the
    shadow; the flat buffer is copied twice in all (shadow -> best state, best state -> model), never swapped."""
    t = rec["trace_driver"][warmup]
    assert t["train"] == rec["trace_plain"], "the driver's epoch differs from a plain run_epoch in its library calls"
    evals = [c for c in t["eval"] if c[0] == "stdadk_eval_indexed_f32"]
    sizes = [BATCH] * (VAL_ROWS // BATCH) + ([VAL_ROWS % BATCH] if VAL_ROWS % BATCH else [])
    assert [c[1] for c in evals] == sizes                                  # one call per batch, last one ragged
    assert [c[3] for c in evals] == pytest.approx([1.0 / b for b in sizes], rel=1e-15)      # 1 / (B Q), Q = 1
    assert [c[0] for c in t["eval"]] == ["stdadk_eval_workspace_bytes"] + ["stdadk_eval_indexed_f32"] * len(sizes)
    assert t["ema_in_place"] and all(t["inside_ema"]) and len(t["inside_ema"]) == len(sizes)
    assert t["flat_copies"] == ["copy_", "copy_"], t["flat_copies"]


def test_argument_errors(rec):
    e = rec["errors"]
    assert e["ok"] == "ok"
    assert "NULL pointer" in e["null_coords"] and "NULL pointer" in e["null_y"]
    assert "workspace" in e["big_B"] and "workspace" in e["small_ws"]
    assert "metric_col" in e["metric_col"] and "metric_col" in e["metric_neg"]
    assert e["null_acc"][0] == -1 and "NULL pointer" in e["null_acc"][1]


def test_optimiser_entry_points_refuse_with_code_and_text(rec):
    """What the AdamW entries and the one-call step refuse, under the prefix of the entry that was called: a clip norm
    without partials, half a non-finite guard, bf16 copies next to a buffer off its 16-byte boundary, an empty group of
    the two-group call (a lone empty group is a no-op), step 0, an incomplete optimiser descriptor."""
    e = rec["optim_errors"]
    assert e["ok"] == "ok" and e["ok2"] == "ok" and e["empty_ok"] == "ok" and e["desc_ok"] == "ok"
    for key, code, text in [
            ("clip", -1, "adamw: max_norm > 0 needs sumsq parts"), ("clip2", -1, "adamw2: max_norm > 0 needs sumsq parts"),
            ("watch", -1, "adamw: loss_watch and nonfinite_step go together (both or neither)"),
            ("watch2", -1, "adamw2: loss_watch and nonfinite_step go together (both or neither)"),
            ("shadow", -3, "adamw: bf16 shadows need 16-byte aligned buffers"),
            ("shadow2", -3, "adamw2: bf16 shadows need 16-byte aligned buffers"),
            ("empty2", -1, "adamw2: NULL pointer or empty group"), ("step0", -1, "adamw: step must be >= 1"),
            ("desc_no_step", -1, "train_step: optimiser descriptor incomplete"),
            ("desc_no_m", -1, "train_step: optimiser descriptor incomplete"),
            ("desc_clip", -1, "train_step: max_norm > 0 needs sumsq_parts")]:
        assert e[key].endswith(f"failed (code {code}): {text}"), (key, e[key])


_DOORS = ("train_fwd_bwd", "train_fwd_bwd_indexed", "train_step", "train_step_next")
_NULL, _BF16, _IDX = "train_fwd_bwd: NULL pointer", ("step: STDADK_FLAG_BF16 needs the fused tail kernels (hidden widths "
                                                     "multiples of 16 up to 256, out_dim <= 8)"), (
    "train_fwd_bwd_indexed: only the window path gathers in place; use stdadk_gather_batch_f32 + "
    "stdadk_train_fwd_bwd_f32 for the materialising path")


def test_step_doors_refuse_with_code_and_text(rec):
    """What the step opener and the four training doors refuse, by error code and text: NULL descriptors, a bad batch
    size, a workspace that is NULL, off its 16-byte boundary or too small, bf16 without the fused tail, NULL parameter /
    gradient tables and observations, a bad loss descriptor, STDADK_FLAG_PREBINNED or idx off the window path, idx or
    next_binned NULL where the door needs them, next_y_cols out of range, and the next batch's own workspace."""
    e = rec["step_errors"]
    for door in _DOORS:
        assert e[door + ":ok"] == [0, ""], (door, e[door + ":ok"])
        for key, code, text in [
                ("null_desc", -1, "mlp: desc is NULL"), ("null_basis", -1, "basis desc is NULL"), ("bad_B", -1, "step: bad B"),
                ("null_ws", -3, "step: workspace NULL or not 16-byte aligned"),
                ("ws_misaligned", -3, "step: workspace NULL or not 16-byte aligned"), ("bf16_no_tail", -1, _BF16),
                ("null_P", -1, _NULL), ("null_G", -1, _NULL), ("null_coords", -1, _NULL),
                ("bad_loss", -1, "loss: y_cols=3 must be 1 or Q=1")]:
            assert e[f"{door}:{key}"] == [code, text], (door, key, e[f"{door}:{key}"])
        code, text = e[door + ":ws_small"]
        assert code == -4 and text.startswith("step: workspace 256 < ") and text.endswith(" bytes"), (door, text)
    # without targets: the step doors refuse; a step that announces its next batch is asked for them by that batch first
    assert e["train_fwd_bwd:null_y"] == e["train_fwd_bwd_indexed:null_y"] == e["train_step:null_y"] == [-1, _NULL]
    no_y = [-1, "train_step: next_y_cols=1 must be in 0..Q with y given"]
    assert e["train_step_next:null_y"] == no_y and e["train_step_next:y_cols_no_y"] == no_y
    for door in ("train_fwd_bwd", "train_step"):
        assert e[door + ":prebinned_dense"] == [-1, "step: STDADK_FLAG_PREBINNED needs the window path"]
        assert e[door + ":prebinned_window_ok"] == [0, ""]       # a binned workspace needs no observations
    assert e["train_step:idx_dense"] == [-1, _IDX] and e["train_fwd_bwd_indexed:idx_dense"] == [-1, _IDX]
    assert e["train_fwd_bwd_indexed:null_idx"] == [-1, "train_fwd_bwd_indexed: idx is NULL"]
    assert e["train_fwd_bwd_indexed:null_idx_B0"] == [0, ""]
    assert e["train_step_next:null_binned"] == [-1, "train_step_next: next_binned is NULL"]
    assert e["train_step_next:no_optim"] == [-1, "train_step: optimiser descriptor incomplete"]
    for key, n in (("y_cols_high", 2), ("y_cols_neg", -1)):
        assert e["train_step_next:" + key] == [-1, f"train_step: next_y_cols={n} must be in 0..Q with y given"]
    code, text = e["train_step_next:next_ws_small"]
    assert code == -4 and text.startswith("step: workspace 256 < ")
    assert e["train_step_next:next_ws_misaligned"] == [-3, "step: workspace NULL or not 16-byte aligned"]
    assert e["train_step_next:next_B_bad"] == [-1, "step: bad B"]
    # covariates: every door asks for X when p > 0, except on a workspace that already holds the binned batch
    for door in _DOORS:
        assert e[door + ":p2_ok"] == [0, ""], (door, e[door + ":p2_ok"])
        assert e[door + ":p2_null_X"] == [-1, "train_fwd_bwd: X is NULL with p=2"], (door, e[door + ":p2_null_X"])
        assert e[door + ":p2_null_X_prebinned"] == [0, ""], (door, e[door + ":p2_null_X_prebinned"])
    # next_binned: 1 after a call that binned, cleared by a call that failed
    assert e["train_step_next:binned_flag"] == [0, 1] and e["train_step_next:binned_reset_on_error"] == [-1, 0]


def test_step_doors_report_the_first_of_two_mistakes(rec):
    """A call with two mistakes reports the one the door checks first: the opener's workspace check before a NULL
    parameter table, the NULL table before the loss descriptor, idx off the window path before the NULL table, a door's
    own argument before anything the shared code checks, the next batch's workspace before this batch's pointers."""
    e = rec["step_errors"]
    for door in _DOORS:
        assert e[door + ":ws_small+null_P"] == e[door + ":ws_small"] and e[door + ":ws_small"][0] == -4
        assert e[door + ":null_P+bad_loss"] == [-1, _NULL]
        assert e[door + ":p2_null_X+bad_loss"] == [-1, "train_fwd_bwd: X is NULL with p=2"]
        assert e[door + ":p2_null_X+null_coords"] == [-1, _NULL]
        assert e[door + ":p2_null_X+ws_small"][0] == -4 and e[door + ":p2_null_X+ws_small"][1].startswith("step: workspace 256 < ")
    assert e["train_step:idx_dense+null_P"] == [-1, _IDX]
    assert e["train_fwd_bwd_indexed:null_idx+null_P"] == [-1, "train_fwd_bwd_indexed: idx is NULL"]
    assert e["train_step_next:null_binned+no_optim"] == [-1, "train_step_next: next_binned is NULL"]
    assert e["train_step_next:next_ws_small+null_P"] == e["train_step_next:next_ws_small"]


if __name__ == "__main__":
    _record(sys.argv[1])
