"""The NEXT batch of a one-call step binned inside the merged weight-gradient launch (dw_all_kernel carrying
bin_dw_body: 256-thread workgroups, the binning image in the launch's static LDS block) instead of inside the
optimiser launch.

Three carriers do the same integer work on the same inputs:
  * `dw`    -- binning workgroups of the weight-gradient launch, plain optimiser launch (the default);
  * `adam`  -- STDADK_BIN_IN=adam: binning workgroups of the optimiser launch (adamw_bin_kernel), also the fallback
               whenever the merged weight-gradient launch is not what the step runs;
  * `side`  -- TrainStep(inline_prep=False): stdadk_bin_batch_f32 on the side stream.
The bins are integers and copies of floats (bit-identical whatever the carrier), and neither the weight gradients nor
the optimiser's arithmetic depend on the shape of the launch that carries the binning, so runs of one-call steps with
announced next batches end in torch.equal parameters and step counters; the loss sums are float atomics and agree to
1e-6 relative (the bound of tests/test_gpu_round3.py::test_next_batch_binned_inside_the_optimiser_launch)."""
import numpy as np
import pytest
import torch

from golden import cases

import test_gpu_parity as T

pytestmark = pytest.mark.gpu

CARRIERS = ("dw", "adam", "side")


def _set_carrier(monkeypatch, carrier):
    if carrier == "adam":
        monkeypatch.setenv("STDADK_BIN_IN", "adam")
    else:
        monkeypatch.delenv("STDADK_BIN_IN", raising=False)


def _model(kind):
    """(model, engine keywords, p) of a case kind."""
    if kind == "c2":
        return T.build_model(cases.MODEL_CASES["c2_b257"], dropout=0.1), {}, 0
    if kind == "k227":
        return T.build_model(cases.MODEL_CASES["default227"], dropout=0.1), {}, 0
    if kind == "q5":
        m, cfg, lc = T.build_quantile_model("default227_mq5")
        return m, dict(loss="pinball", quantile_levels=lc["taus"], non_crossing_weight=0.5), 0
    if kind == "p2":
        return T.build_model(dict(cases.MODEL_CASES["default227"], p=2), dropout=0.1), {}, 2
    raise KeyError(kind)


def _data(n, Q, p, seed):
    rs = np.random.RandomState(seed)
    d = T.dev()
    coords = torch.from_numpy(rs.uniform(0, 1, (n, 2)).astype(np.float32)).to(d)
    t = torch.from_numpy(rs.uniform(0, 1, (n,)).astype(np.float32)).to(d)
    y = torch.from_numpy(rs.standard_normal((n, Q)).astype(np.float32)).to(d)
    X = torch.from_numpy(rs.standard_normal((n, p)).astype(np.float32)).to(d) if p else None
    return coords, t, y, X


def _run(monkeypatch, kind, batches, dtype, data):
    """Parameters, mean loss and step counter after one-call steps over `batches`, one result per carrier.  A next batch
    of up to 4 096 rows (at most 64 x 64 cells) is binned inside the step; a larger one the library declines and the
    engine prepares it on the side stream."""
    from stnf.engine import TrainStep
    coords, t, y, X = data
    B = max(b.numel() for b in batches)
    res = {}
    for carrier in CARRIERS:
        _set_carrier(monkeypatch, carrier)
        m, kw, p = _model(kind)
        m.train()
        eng = TrainStep(m, lr=1e-3, grad_clip=0.5, ema_decay=0.99, max_batch=B, dtype=dtype, seed=11,
                        inline_prep=carrier != "side", **kw)
        assert eng._whole_step and eng.uses_window
        for i, idx in enumerate(batches):
            nxt = batches[i + 1] if i + 1 < len(batches) else None
            eng.step_indexed(coords, t, y, idx, X_all=X, next_idx=nxt)
            if nxt is not None:
                # inline: the library took the next batch (dw / adam); otherwise the engine used the side stream
                assert eng._prepared is not None
                assert eng._prepared.inline == (nxt.numel() <= 4096 and carrier != "side"), (carrier, i)
        torch.cuda.synchronize()
        res[carrier] = (eng.flat.clone(), eng.ema.clone() if eng.ema is not None else None, eng.mean_loss(),
                        int(eng.step_dev.item()))
        del eng, m
    ref = res["side"]
    assert torch.isfinite(ref[0]).all()
    for carrier in ("dw", "adam"):
        got = res[carrier]
        assert got[3] == ref[3] == len(batches), carrier
        assert torch.equal(got[0], ref[0]), carrier
        if ref[1] is not None:
            assert torch.equal(got[1], ref[1]), carrier
        print(f"{kind} {carrier}: loss {got[2]!r} side {ref[2]!r}")
        assert abs(got[2] - ref[2]) <= 1e-6 * abs(ref[2]), carrier


def _perm_batches(n, B, seed, steps=5):
    """`steps` batches of B distinct rows and one ragged last batch."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    perm = torch.randperm(n, generator=g).to(T.dev())
    return [perm[i * B:(i + 1) * B] for i in range(steps)] + [perm[:max(B // 2, 1)]]


@pytest.mark.parametrize("B", [1, 63, 64, 257, 1500, 4096])
def test_batch_sizes_with_a_ragged_last_batch(B, monkeypatch):
    n = 5 * B + 37
    _run(monkeypatch, "c2", _perm_batches(n, B, 5), "f32", _data(n, 1, 0, 21))


def test_index_tensor_with_repeated_rows(monkeypatch):
    """Rows drawn WITH replacement from a few hundred sites: cells hold many equal coordinates and the order inside a
    cell ("ascending batch position") is all that separates them."""
    n, B = 300, 2000
    g = torch.Generator(device="cpu").manual_seed(9)
    batches = [torch.randint(0, n, (B,), generator=g).to(T.dev()) for _ in range(6)]
    _run(monkeypatch, "c2", batches, "f32", _data(n, 1, 0, 22))


@pytest.mark.parametrize("y_cols", [1, 5])
def test_pinball_five_quantiles_carries_target_columns(y_cols, monkeypatch):
    """Q = 5 outputs; targets of one column (the reference's shape) and of five (y_s carries five columns a row)."""
    n, B = 3000, 500
    _run(monkeypatch, "q5", _perm_batches(n, B, 6), "f32", _data(n, y_cols, 0, 23))


def test_covariates_are_carried(monkeypatch):
    n, B = 3000, 500
    _run(monkeypatch, "p2", _perm_batches(n, B, 7), "f32", _data(n, 1, 2, 24))


def test_bf16_operands(monkeypatch):
    n, B = 5 * 4096 + 37, 4096
    _run(monkeypatch, "c2", _perm_batches(n, B, 8), "bf16", _data(n, 1, 0, 25))


def test_227_knot_model_on_the_window_path(monkeypatch):
    n, B = 4000, 700
    _run(monkeypatch, "k227", _perm_batches(n, B, 10), "f32", _data(n, 1, 0, 26))


def test_6000_rows_take_the_fallback(monkeypatch):
    """More rows than the binning workgroups of either launch hold (a 128 x 128 cell grid): the library declines
    (*next_binned == 0) whatever the switch says and the engine prepares on the side stream; the ragged last batch
    (3 000 rows) is binned inside a 6 000-row step.  Same results."""
    n, B = 5 * 6000 + 37, 6000
    _run(monkeypatch, "c2", _perm_batches(n, B, 12), "f32", _data(n, 1, 0, 27))


@pytest.mark.parametrize("carrier,no_dw_all,want", [("dw", False, "dw"), ("adam", False, "adam"), ("dw", True, "adam")])
def test_the_switch_selects_the_carrier(carrier, no_dw_all, want, monkeypatch):
    """Which launches a step makes (the library's own launch record): with the binning in the weight-gradient launch the
    optimiser is the plain adamw_ema_kernel; STDADK_BIN_IN=adam, or a step that does not run the merged launch
    (STDADK_NO_DW_ALL=1), bins in adamw_bin_kernel exactly as before -- and the next batch is binned either way."""
    from stnf import _native as N
    from stnf.engine import TrainStep
    _set_carrier(monkeypatch, carrier)
    if no_dw_all:
        monkeypatch.setenv("STDADK_NO_DW_ALL", "1")
    n, B = 3 * 4096, 4096
    coords, t, y, X = _data(n, 1, 0, 28)
    batches = _perm_batches(n, B, 13, steps=3)
    m, kw, p = _model("c2")
    eng = TrainStep(m.train(), lr=1e-3, grad_clip=0.5, ema_decay=0.99, max_batch=B, seed=11)
    eng.step_indexed(coords, t, y, batches[0], next_idx=batches[1])
    torch.cuda.synchronize()
    N.profile_enable(True)
    try:
        eng.step_indexed(coords, t, y, batches[1], next_idx=batches[2])
        names = [k for k, _ in N.profile_collect()]
    finally:
        N.profile_enable(False)
    assert eng._prepared is not None and eng._prepared.inline
    if want == "dw":
        assert "adamw_bin_kernel" not in names and "adamw_ema_kernel" in names and "dw_all_kernel" in names, names
        assert "bin_small_kernel" not in names, names
    else:
        assert "adamw_bin_kernel" in names and "adamw_ema_kernel" not in names, names
