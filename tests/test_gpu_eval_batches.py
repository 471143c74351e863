"""The validation pass per batch, stdadk_eval_indexed_f32, against float64 at the batch sizes, heads, index shapes and
accumulator states real runs give it (tests/test_gpu_validation.py runs it at 1000 rows in batches of 300 only).

Cases, the float64 reference, the comparator and the reduction bound: golden/eval_cases.py; that the bound holds for
the kernel's order of operations and that the comparator catches the ways the pass can go wrong:
tests/test_eval_cases_cpu.py.  Two comparisons per call, kept apart so that each bound stays tight:
  * every accumulator slot against float64 sums over the predictions the call RETURNED and the targets at idx, within
    the reduction bound (a + 6 + c) 2^-24 sum|term|; ROWS and BATCHES exact; unused slots bit-identical;
  * the returned predictions, row b against the float64 oracle's forward of row idx[b], within the project's forward
    bound: 1e-5 of max(1, max|y|) (test_gpu_mlp_shapes.test_predictor_against_float64).

Routes.  The window kernels need a first hidden layer of 128 or 256 units (window.hip, l1_window_supported): `tiny9`
(32 units) runs the materialising kernels whatever `force_window_path` says.  So "window" is tiny9 / tiny9_ln_p3 with
hidden_dims [128, 16] (asserted to take the window path: binning, predictions through the un-permute, targets carried
into sorted order), "dense" is tiny9 under FLAG_DENSE, and "asked" is tiny9 with force_window_path as it stands (the
library's own choice: the materialising path with the first weight transposed).  The planted rows of make_rows sit
where the metrics kernel's loops can lose a row IN THE ORDER IT READS THEM: the caller's on "dense" and "asked", the
binned order on "window" (eval_cases.binned_order, compared with the library's own permutation below).

The production calls (C2 model, 32 768 and 65 536 + 300 rows) go through Evaluator.evaluate against metrics from the
chunked float64 forward of oracle/torch_f64.py on the GPU, at the 1e-5 relative of test_gpu_validation.py."""
import math

import numpy as np
import pytest
import torch

from golden import cases
from golden import eval_cases as ec
from oracle import stdadk_oracle as orc
from oracle import torch_f64
from test_gpu_parity import build_model, build_quantile_model, dev

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROUTES = ("window", "dense", "asked")
_MODELS, _PROD = {}, {}


class _Entry:
    pass


def _model(base, Q, route):
    """One model per (base case, output width, route) with its eval-mode step descriptors, shared by the tests."""
    from stnf import _native as N
    key = (base, Q, route)
    if key not in _MODELS:
        cfg = dict(cases.MODEL_CASES[base], output_dim=Q, seed=cases.MODEL_CASES[base]["seed"] + 100 * Q)
        if route == "window":
            cfg["hidden_dims"] = [128, 16]
        e = _Entry()
        e.cfg, e.model = cfg, build_model(cfg).eval()
        assert e.model.force_window_path
        e.st = e.model._step_state(dev(), force_dense=(route == "dense"), training=False)
        e.window = bool(N.step_uses_window(e.st.basis, e.st.desc, e.st.flags))
        assert e.window == (route == "window"), (key, e.window)
        e.params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
        _MODELS[key] = e
    return _MODELS[key]


def _loss_desc(head):
    from stnf import _native as N
    if head["kind"] == "mse_null":
        return None
    return N.make_loss("pinball" if head["kind"] == "pinball" else "mse", head["Q"], head["y_cols"],
                       [float(x) for x in ec.head_taus(head)], head["nc_weight"], head["nc_power"])


class _Batch:
    """The resident arrays of one make_rows() on the device, and the raw call on them."""

    def __init__(self, ent, head, rows):
        d = dev()
        self.ent, self.head, self.rows = ent, head, rows
        self.coords = torch.from_numpy(rows["coords"]).to(d)
        self.t = torch.from_numpy(rows["t"]).to(d).view(-1)
        self.X = torch.from_numpy(rows["X"]).to(d) if ent.cfg["p"] > 0 else None
        self.y = torch.from_numpy(rows["y"]).to(d)
        self.idx = torch.from_numpy(rows["idx"]).to(d)
        self.ldesc = _loss_desc(head)
        self.ws = None

    def call(self, acc, yp, weight):
        from stnf import _native as N
        st = self.ent.st
        if self.ws is None:
            need = N.eval_workspace_bytes(st.basis, st.desc, self.idx.numel(), st.flags)
            self.ws = torch.empty((need + 3) // 4, device=dev())
        N.eval_indexed(st.basis, st.desc, st.params, self.coords, self.t, self.X, self.y, self.idx, self.ldesc,
                       self.head["metric_col"], weight, acc, yp, self.ws, st.flags)

    def set_targets(self, y):
        self.rows["y"] = y
        self.y.copy_(torch.from_numpy(y))


def _prepare(base, route, head, B, kind, seed):
    """make_rows on the device, one call for the predictions, the ties set from them.  Returns (batch, yp) with yp the
    float32 predictions (B, Q) on the host, in the caller's order."""
    ent = _model(base, head["Q"], route)
    rows = ec.make_rows(B, head["Q"], head["y_cols"], seed, kind, cfg=ent.cfg, binned=ent.window)
    bt = _Batch(ent, head, rows)
    yp = torch.full((B, head["Q"]), float("nan"), device=dev())
    bt.call(torch.zeros(ec.EVAL_SLOTS, dtype=torch.float64, device=dev()), yp, 1.0)
    yp_h = yp.cpu().numpy()
    assert np.all(np.isfinite(yp_h))
    if rows["ties"]:
        y = rows["y"].copy()
        ec.set_ties(y, rows["idx"], yp_h, rows["ties"])
        bt.set_targets(y)
    return bt, yp_h


def _check_call(what, bt, yp_first, weight=None, planted=True):
    """One call from a zero accumulator with a prediction buffer: every slot within the reduction bound, ROWS == B and
    BATCHES == 1 exactly, the predictions the same bits as the first call's (they do not depend on the targets), the
    ties hit exactly.  Returns the predictions."""
    head, rows = bt.head, bt.rows
    B, Q = len(rows["idx"]), head["Q"]
    w = 1.0 / (B * Q) if weight is None else weight
    acc = torch.zeros(ec.EVAL_SLOTS, dtype=torch.float64, device=dev())
    yp = torch.full((B, Q), float("nan"), device=dev())
    bt.call(acc, yp, w)
    got, yp_h = acc.cpu().numpy(), yp.cpu().numpy()
    assert np.array_equal(yp_h, yp_first), f"{what}: the predictions of two calls on the same rows differ"
    y_at = rows["y"][rows["idx"]]
    for b in rows["ties"]:
        assert np.any(y_at[b] == yp_h[b]), (what, "tie", b)
    add, _, bound = ec.reference(yp_h, y_at, head, w)
    failures, worst = ec.compare_accumulator(got, np.zeros(ec.EVAL_SLOTS), add, bound, Q)
    names = ec.slot_names(Q)
    at = max((s for s in names if bound[s] > 0), key=lambda s: abs(got[s] - add[s]) / bound[s], default=ec.EVAL_SSE)
    share = ec.planted_shares(yp_h, y_at, head, rows["planted"]) if planted else float("nan")
    print(f"{what}: worst slot {names[at]} err {abs(got[at] - add[at]):.3g} bound {bound[at]:.3g} "
          f"({worst:.3f} of the bound), planted share {share:.3g}")
    assert got[ec.EVAL_ROWS] == B and got[ec.EVAL_BATCHES] == 1.0
    assert not failures, (what, failures, [(names.get(s, s), got[s], add[s], bound[s]) for s in range(ec.EVAL_SLOTS)])
    if planted:
        assert share >= ec.PLANTED_SHARE, (what, share)
    return yp_h


def _check_forward(what, bt, yp_h):
    """y_pred[b] against the float64 oracle's forward of row idx[b]: every row, or FORWARD_SAMPLE sampled rows plus the
    planted and tie rows from BIG rows on."""
    rows, cfg = bt.rows, bt.ent.cfg
    B = len(rows["idx"])
    if B >= ec.BIG:
        pick = np.random.RandomState(B % 7919).choice(B, ec.FORWARD_SAMPLE, replace=False)
        pick = np.unique(np.concatenate([pick, np.array(rows["planted"] + rows["ties"], dtype=np.int64)]))
    else:
        pick = np.arange(B)
    src = rows["idx"][pick]
    yo = orc.model_forward(rows["X"][src], rows["coords"][src], rows["t"][src], bt.ent.params, cfg)[0]
    scale = max(1.0, float(np.abs(yo).max()))
    diff = np.abs(yp_h[pick].astype(np.float64) - yo)
    b = int(np.argmax(diff.max(axis=1)))
    err = float(diff.max()) / scale
    print(f"{what}: forward max-abs {err:.2e} of max(1, max|y|) over {len(pick)} rows (worst: batch row {pick[b]} <- "
          f"resident row {src[b]})")
    assert err <= TOL, (what, err, int(pick[b]), int(src[b]))


def _rotate(i, r):
    return ec.HEADS[(5 * i + 6 * r) % len(ec.HEADS)]


# ------------------------------------------------------------------ the reduction: every slot, every batch size
@pytest.mark.parametrize("B", ec.BATCH_SIZES)
@pytest.mark.parametrize("route", ROUTES)
def test_reduction_every_slot_every_batch_size(route, B):
    i, r = ec.BATCH_SIZES.index(B), ROUTES.index(route)
    head = _rotate(i, r)
    kind = ec.INDEX_KINDS[(i + r) % 4]                     # arange, reversed, permutation, subset: no repeats
    what = f"{route} B={B} {head['name']} {kind}"
    bt, yp0 = _prepare("tiny9", route, head, B, kind, seed=200 + i)
    yp = _check_call(what, bt, yp0)
    _check_forward(what, bt, yp)


@pytest.mark.parametrize("B", [257, 65537, 1048576])
def test_binned_order_is_the_librarys(B):
    """eval_cases.binned_order, which places the planted rows on the window route, against stdadk_bin_obs_f32 on the
    same coordinates with the step's own grid (integers: bit-exact)."""
    from stnf import _native as N
    rows = ec.make_rows(B, 1, 1, seed=250, kind="permutation")
    at = np.ascontiguousarray(rows["coords"][rows["idx"]])
    _, _, perm = N.bin_obs(torch.from_numpy(at).to(dev()), ec.cell_grid(B))
    assert np.array_equal(perm.cpu().numpy().astype(np.int64), ec.binned_order(at, B))


def test_the_largest_batches_see_the_widest_heads():
    """Across the routes, the sizes whose threads make several trips meet a Q = 8 head, a pinball penalty and a
    broadcast target (the rotation above, restated so that a change of the tables cannot lose it)."""
    for B in (262145, 1048576):
        heads = [_rotate(ec.BATCH_SIZES.index(B), r) for r in range(len(ROUTES))]
        assert any(h["Q"] == ec.MAX_Q for h in heads), [h["name"] for h in heads]
        assert any(h["kind"] == "pinball" for h in heads) and any(h["y_cols"] == 1 for h in heads)


# ------------------------------------------------------------------ predictions in the caller's order
@pytest.mark.parametrize("B", [257, 1023])
@pytest.mark.parametrize("kind", ec.INDEX_KINDS)
@pytest.mark.parametrize("base,route", [("tiny9", "window"), ("tiny9", "dense"), ("tiny9_ln_p3", "window"),
                                        ("tiny9_ln_p3", "dense")])
def test_predictions_in_callers_order(base, route, kind, B):
    k = ec.INDEX_KINDS.index(kind)
    head = _rotate(k + (B == 1023), 1 + (base != "tiny9"))
    what = f"{base} {route} B={B} {kind} {head['name']}"
    bt, yp0 = _prepare(base, route, head, B, kind, seed=300 + k)
    yp = _check_call(what, bt, yp0, planted=kind not in ("all_same", "few_repeated"))
    _check_forward(what, bt, yp)
    if kind == "all_same":
        assert np.all(yp == yp[0])
    if kind == "few_repeated":
        assert np.array_equal(yp[7:14], yp[:7])


# ------------------------------------------------------------------ every head
@pytest.mark.parametrize("head", ec.HEADS, ids=[h["name"] for h in ec.HEADS])
@pytest.mark.parametrize("route", ["window", "dense"])
def test_every_head(route, head):
    what = f"{route} B=1023 {head['name']}"
    bt, yp0 = _prepare("tiny9", route, head, 1023, "permutation", seed=400)
    yp = _check_call(what, bt, yp0)
    _check_forward(what, bt, yp)


def _expected(yp, y, batch, taus=None, nc_weight=0.0, nc_power=1):
    """test_gpu_validation._expected extended to column targets: every key of Evaluator.evaluate in numpy float64 from
    float64 predictions yp (N, Q) and targets y (N, 1) or (N, Q)."""
    yp, y = np.asarray(yp, np.float64), np.asarray(y, np.float64)
    n, Q = yp.shape
    yt = np.broadcast_to(y, (n, Q)) if y.shape[1] == 1 else y
    d = yp[:, Q // 2] - yt[:, Q // 2]
    out = {"mse": np.mean(d ** 2), "mae": np.mean(np.abs(d))}
    out["rmse"] = math.sqrt(out["mse"])
    per_batch = []
    for s in range(0, n, batch):
        pb, yb = yp[s:s + batch], yt[s:s + batch]
        if taus is None:
            per_batch.append(np.mean((pb - yb) ** 2))
        else:
            e = yb - pb
            tq = np.asarray(taus, np.float64)[None, :]
            obj = np.mean(np.maximum((tq - 1) * e, tq * e))
            if nc_weight > 0 and Q > 1:
                g = np.maximum(pb[:, :-1] - pb[:, 1:], 0.0)
                obj += nc_weight * np.mean(np.sum(g if nc_power == 1 else g * g, axis=1))
            per_batch.append(obj)
    out["loss"] = float(np.mean(per_batch))
    if taus is not None:
        e = yt - yp
        tq = np.asarray(taus, np.float64)[None, :]
        checks = np.mean(np.maximum((tq - 1) * e, tq * e), axis=0)
        if Q == 1:
            out["check_loss"] = float(checks[0])
        else:
            out["mean_check_loss"] = out["check_loss"] = float(np.mean(checks))
            out["crps"] = 2.0 * float(np.mean(checks))
    return out


def _compare(got, want, rows, what):
    for k, w in want.items():
        print(f"{what}: {k} got {got[k]:.12g} float64 {w:.12g} rel {abs(got[k] - w) / max(abs(w), 1e-300):.3g}")
    assert got["rows"] == rows
    assert set(want) <= set(got)
    for k, w in want.items():
        assert abs(got[k] - w) <= TOL * abs(w), (what, k, got[k], w)


def _dataset(rows, cfg, n=None):
    from stnf.dataio.device_dataset import DeviceDataset
    d = dev()
    n = len(rows["coords"]) if n is None else n
    return DeviceDataset(torch.from_numpy(rows["coords"][:n]).to(d), torch.from_numpy(rows["t"][:n]).to(d),
                         torch.from_numpy(rows["y"][:n]).to(d),
                         torch.from_numpy(rows["X"][:n]).to(d) if cfg["p"] > 0 else None)


@pytest.mark.parametrize("loss", ["mse", "pinball"])
@pytest.mark.parametrize("route", ["window", "dense"])
def test_evaluator_with_column_targets(route, loss):
    """A DeviceDataset whose y has Q = 5 columns through Evaluator: MSE (Evaluator._loss_desc gives None: the NULL
    descriptor) and pinball with the power-2 penalty, 1000 rows in batches of 300."""
    from stnf.evaluation import Evaluator
    Q, n, batch = 5, 1000, 300
    ent = _model("tiny9", Q, route)
    rows = ec.make_rows(n, Q, Q, seed=500)
    taus = cases.TAUS5 if loss == "pinball" else None
    ev = Evaluator(ent.model, loss=loss, quantile_levels=taus, non_crossing_weight=2.0, non_crossing_power=2,
                   max_batch=batch, force_dense=(route == "dense"))
    assert (ev._loss_desc(Q) is None) == (loss == "mse")
    got = ev.evaluate(_dataset(rows, ent.cfg), batch)
    yo = orc.model_forward(rows["X"], rows["coords"], rows["t"], ent.params, ent.cfg)[0]
    _compare(got, _expected(yo, rows["y"], batch, taus, 2.0, 2), n, f"{route} {loss} column targets")
    assert ev.sums[ec.EVAL_BATCHES] == 4.0


# ------------------------------------------------------------------ the accumulator contract
def _two_calls(bts, acc, weights):
    for bt, w in zip(bts, weights):
        bt.call(acc, None, w)
    return acc.cpu().numpy()


@pytest.mark.parametrize("route", ["window", "dense"])
def test_accumulator_contract(route):
    """The pass ADDS: sentinels in all 16 slots, two calls of different sizes and weights, no prediction buffer.  Used
    slots = sentinel + call 1 + call 2 within the summed bounds, ROWS and BATCHES exact sums, slots from CHECK + Q on
    bit-identical to their sentinels; the weight scales OBJECTIVE only; the same calls again give the same bits."""
    head = ec.HEADS[6]                                       # Q = 5: slots 10..15 are unused
    Q = head["Q"]
    weights = (0.37, 1.9)
    prep = [_prepare("tiny9", route, head, B, "permutation", seed=600 + B) for B in (257, 65537)]
    bts = [p[0] for p in prep]
    start = np.array([3.25 + 1.5 * s for s in range(ec.EVAL_SLOTS)])
    start[ec.EVAL_ROWS], start[ec.EVAL_BATCHES] = 1000.0, 7.0
    add, bound = np.zeros(ec.EVAL_SLOTS), np.zeros(ec.EVAL_SLOTS)
    for (bt, yp), w in zip(prep, weights):
        a, _, b = ec.reference(yp, bt.rows["y"][bt.rows["idx"]], head, w)
        add, bound = add + a, bound + b

    def run(ws):
        return _two_calls(bts, torch.from_numpy(start.copy()).to(dev()), ws)

    got = run(weights)
    failures, worst = ec.compare_accumulator(got, start, add, bound, Q)
    print(f"{route}: sentinels + 257 rows + 65537 rows: worst {worst:.3f} of the bound; slots {got.tolist()}")
    assert not failures, (failures, got, start + add)
    assert got[ec.EVAL_ROWS] == 1000.0 + 257 + 65537 and got[ec.EVAL_BATCHES] == 9.0
    assert np.array_equal(got[ec.EVAL_CHECK + Q:].view(np.int64), start[ec.EVAL_CHECK + Q:].view(np.int64))
    again = run(weights)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), "the same two calls give other bits"
    # four times the weight (exact in binary): OBJECTIVE's additions scale, every other slot keeps its bits
    scaled = run(tuple(4.0 * w for w in weights))
    others = [s for s in range(ec.EVAL_SLOTS) if s != ec.EVAL_OBJECTIVE]
    assert np.array_equal(scaled[others].view(np.int64), got[others].view(np.int64))
    d1, d4 = got[ec.EVAL_OBJECTIVE] - start[0], scaled[ec.EVAL_OBJECTIVE] - start[0]
    assert abs(d4 - 4.0 * d1) <= 8.0 * bound[ec.EVAL_OBJECTIVE], (d1, d4)
    assert abs(d4 - 4.0 * add[ec.EVAL_OBJECTIVE]) <= 4.0 * bound[ec.EVAL_OBJECTIVE]


@pytest.mark.parametrize("head", [ec.HEADS[6], ec.HEADS[7], ec.HEADS[12]], ids=lambda h: h["name"])
@pytest.mark.parametrize("route", ["window", "dense"])
def test_nan_target_is_not_dropped(route, head):
    """One NaN target (batch position 100, column 0): exactly the slots the float64 numpy reference makes NaN are NaN
    -- with one broadcast column all of OBJECTIVE, SSE, SAE and CHECK; with column targets OBJECTIVE, CHECK[0] and,
    where metric_col is 0, SSE and SAE -- the others stay inside their bounds, ROWS and BATCHES exact."""
    B, Q = 1023, head["Q"]
    bt, yp0 = _prepare("tiny9", route, head, B, "permutation", seed=700)
    y = bt.rows["y"].copy()
    y[bt.rows["idx"][100], 0] = np.nan
    bt.set_targets(y)
    acc = torch.zeros(ec.EVAL_SLOTS, dtype=torch.float64, device=dev())
    w = 1.0 / (B * Q)
    bt.call(acc, None, w)
    got = acc.cpu().numpy()
    add, _, bound = ec.reference(yp0, y[bt.rows["idx"]], head, w)
    names = ec.slot_names(Q)
    nan_ref = sorted(names[s] for s in names if np.isnan(add[s]))
    nan_got = sorted(names[s] for s in names if np.isnan(got[s]))
    print(f"{route} {head['name']}: NaN slots {nan_got}; float64 reference {nan_ref}")
    assert "objective" in nan_ref and "check0" in nan_ref and "rows" not in nan_ref
    if head["y_cols"] == 1:
        assert set(nan_ref) == set(names.values()) - {"rows", "batches"}
    else:
        assert ("sse" in nan_ref) == (head["metric_col"] == 0) and "check1" not in nan_ref
    assert nan_got == nan_ref
    assert ec.compare_accumulator(got, np.zeros(ec.EVAL_SLOTS), add, bound, Q)[0] == []
    assert got[ec.EVAL_ROWS] == B and got[ec.EVAL_BATCHES] == 1.0


# ------------------------------------------------------------------ the production validation calls
PROD_ROWS = 65536 + 300


def _production(name):
    """(model, cfg, loss spec, host arrays of PROD_ROWS rows, float64 predictions), once per model."""
    if name not in _PROD:
        if name == "c2_b257":
            cfg, lc = dict(cases.MODEL_CASES[name]), None
            m = build_model(cfg)
        else:
            m, cfg, lc = build_quantile_model(name)
        m.eval()
        X, coords, t, y = cases.make_inputs(dict(cfg, B=PROD_ROWS, seed=cfg["seed"] + 900))
        params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
        yo = torch_f64.forward(X, coords, t, params, cfg, device=dev(), chunk=4096)
        _PROD[name] = (m, cfg, lc, dict(X=X, coords=coords, t=t, y=y), yo)
    return _PROD[name]


def _prod_evaluator(m, lc, dense, max_batch=65536):
    from stnf.evaluation import Evaluator
    if lc is None:
        return Evaluator(m, max_batch=max_batch, force_dense=dense)
    return Evaluator(m, loss="pinball", quantile_levels=lc["taus"], non_crossing_weight=lc["nc_weight"],
                     non_crossing_power=lc["nc_power"], max_batch=max_batch, force_dense=dense)


@pytest.mark.parametrize("n,batch,headline", [(32768, 32768, 1024), (PROD_ROWS, 65536, 4096)])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", ["c2_b257", "c2_b257_mq3"])
def test_production_validation_calls(name, dense, n, batch, headline):
    """train_model's validation call: val_batch_size rows per call of the C2 model -- its floor of 32 768 in one call,
    and the headline batch's 65 536 with a ragged last call of 300 -- f32, both routes."""
    from stnf import _native as N
    from stnf import training as T
    assert T.val_batch_size(headline, n) == batch
    m, cfg, lc, rows, yo = _production(name)
    ev = _prod_evaluator(m, lc, dense)
    got = ev.evaluate(_dataset(rows, cfg, n), batch)
    st = m._step_state(dev(), force_dense=dense, training=False)
    assert bool(N.step_uses_window(st.basis, st.desc, st.flags)) == (not dense)
    kw = {} if lc is None else dict(taus=lc["taus"], nc_weight=lc["nc_weight"], nc_power=lc["nc_power"])
    _compare(got, _expected(yo[:n], rows["y"][:n], batch, **kw), n, f"{name} dense={dense} rows={n}")
    assert ev.sums[ec.EVAL_BATCHES] == math.ceil(n / batch)


def test_bf16_ema_views_equal_ema_swap_at_65536_rows():
    """test_gpu_validation.test_ema_views_equal_ema_swap at the size of a real validation call: C2 model, bf16 matrix
    cores, two steps of the headline batch, then 65 536 rows through views of the shadow and through the swap."""
    from stnf.engine import TrainStep
    from stnf.evaluation import Evaluator
    cfg = dict(cases.MODEL_CASES["c2_b257"])
    _, _, _, rows, _ = _production("c2_b257")
    ds = _dataset(rows, cfg, 65536)
    o = cases.OPT
    eng = TrainStep(build_model(cfg).train(), lr=o["lr"], weight_decay=o["weight_decay"], grad_clip=o["grad_clip"],
                    ema_decay=o["ema_decay"], max_batch=4096, seed=3, dtype="bf16")
    for i in range(2):
        idx = torch.arange(i * 4096, (i + 1) * 4096, device=dev())
        eng.step_indexed(ds.coords, ds.t, ds.y, idx, X_all=ds.X)
    ev = Evaluator(eng.model, max_batch=65536)
    assert Evaluator.ema_in_place(eng)
    r = ev.evaluate(ds, 65536, params="ema", engine=eng)
    in_place = list(ev.sums)
    eng.swap_in_ema()
    ev.evaluate(ds, 65536, params="live", engine=eng)
    swapped = list(ev.sums)
    eng.swap_in_ema()
    live = ev.evaluate(ds, 65536, params="live", engine=eng)
    print("in place", in_place[:5], "swapped", swapped[:5], "live loss", live["loss"])
    assert r["rows"] == 65536 and math.isfinite(r["loss"]) and in_place[ec.EVAL_BATCHES] == 1.0
    assert in_place == swapped
    assert live["loss"] != r["loss"]                       # (the shadow lags the live weights)


# ------------------------------------------------------------------ Evaluator host edges
def _small_set(n=1000):
    ent = _model("tiny9", 1, "window")
    rows = ec.make_rows(n, 1, 1, seed=800)
    return ent, rows, _dataset(rows, ent.cfg)


def test_evaluator_regrows_its_workspace():
    from stnf.evaluation import Evaluator
    ent, rows, ds = _small_set()
    ev = Evaluator(ent.model, max_batch=300)
    ev.evaluate(ds, 300)
    small = {k: w.numel() for k, w in ev._ws.items()}
    ev.evaluate(ds, 1000)
    grown = list(ev.sums)
    assert all(ev._ws[k].numel() > n for k, n in small.items())
    fresh = Evaluator(ent.model, max_batch=1000)
    fresh.evaluate(ds, 1000)
    assert grown == fresh.sums and grown[ec.EVAL_ROWS] == 1000 and grown[ec.EVAL_BATCHES] == 1.0


def test_evaluator_takes_a_list_of_batch_sizes():
    """The data-parallel schedule (DeviceDataset.epoch_batches with a list): the same split gives the same bits; another
    split gives the same per-row sums.  Both runs are within (1 + 6 + 3) 2^-24 of their float64 sums of non-negative
    terms (the reduction bound with one trip per thread, c <= 3), so of each other within twice that."""
    from stnf.evaluation import Evaluator
    ent, rows, ds = _small_set()
    ev = Evaluator(ent.model, max_batch=300)
    ev.evaluate(ds, 300)
    one = list(ev.sums)
    ev.evaluate(ds, [300, 300, 300, 100])
    assert list(ev.sums) == one
    r = ev.evaluate(ds, [250, 449, 1, 300])
    other = list(ev.sums)
    assert r["rows"] == 1000 and other[ec.EVAL_BATCHES] == 4.0 and one[ec.EVAL_ROWS] == other[ec.EVAL_ROWS] == 1000
    for s in (ec.EVAL_SSE, ec.EVAL_SAE, ec.EVAL_CHECK):
        rel = abs(one[s] - other[s]) / one[s]
        print(f"slot {s}: {one[s]!r} in batches of 300, {other[s]!r} in 250 + 449 + 1 + 300: rel {rel:.3g}")
        assert rel <= 2 * (1 + ec.TREE_LEVELS + 3) * ec.ULP
    with pytest.raises(ValueError, match="sum to"):
        ev.evaluate(ds, [300, 300])


def test_evaluator_on_an_empty_dataset(monkeypatch):
    from stnf import _native as N
    from stnf.dataio.device_dataset import DeviceDataset
    from stnf.evaluation import Evaluator
    ent, rows, ds = _small_set()
    ev = Evaluator(ent.model, max_batch=300)
    ev.evaluate(ds, 300)                                     # (a non-zero accumulator to start from)
    assert ev.sums[ec.EVAL_ROWS] == 1000

    def refuse(*a, **k):
        raise AssertionError("a launch for an empty dataset")

    monkeypatch.setattr(N, "eval_indexed", refuse)
    d = dev()
    empty = DeviceDataset(torch.empty(0, 2, device=d), torch.empty(0, 1, device=d), torch.empty(0, 1, device=d))
    r = ev.evaluate(empty, 300)
    assert r["rows"] == 0 and ev.sums == [0.0] * ec.EVAL_SLOTS
    assert r["loss"] == 0.0 and r["mse"] == 0.0
