"""Large-batch one-call steps (TrainStep.step, the path bench.py times) against a float64 reference, and the
next-batch planning of the one-call step at the edge of its workspace.

The dense numpy oracle cannot hold these batches; the reference here is its chunked float64 torch restatement
(oracle/torch_f64.py, pinned against the numpy oracle in tests/test_torch_f64_oracle.py), evaluated on the GPU.

Batch sizes (C2 model, f32, dropout 0):
  * 12 289: 32-row tail tiles (tail.hip, tail_rows: 8 192 <= B < 16 384), a ragged last tile;
  * 16 384: the first 64-row tiles, a batch_sweep point;
  * 49 151 / 49 152: either side of FIN_FULL_MIN_ROWS (mlp.hip), where the weight-gradient launch starts doing
    the reductions itself (arrival counters, last K slice sums the slabs);
  * 65 536: a batch_sweep point and the weak-scaling line's batch;
  * STDADK_DW_FIN forces the other finishing mode at 49 151 (-> 2) and 65 536 (-> 1);
  * C4 (49 728 knots) at 16 384 rows: the weak-scaling line's per-rank shape, gradients only.
"""
import os

import numpy as np
import pytest
import torch

from golden import cases
from oracle import stdadk_oracle as orc
from oracle import torch_f64

import test_gpu_parity as T
import test_gpu_round2 as R2

pytestmark = pytest.mark.gpu
TOL = 1e-5
KINK_TOL = 1e-6

C4 = dict(p=0, k_spatial_centers=[1024, 4096, 16384, 28224], k_temporal_centers=[10, 15, 45],
          hidden_dims=[256, 256, 128], layernorm=True, basis="wendland", output_dim=1, seed=62)
CONFIGS = {"c2": cases.MODEL_CASES["c2_b257"], "c4": C4}

# hidden units within KINK_TOL of a ReLU kink that a case's fp32 step may take from the other side (fitted from the
# residual, orc.fit_kink_sides): bounded per case from the recorded counts (12 289: 0 of 4 near-kink units,
# 16 384: 1 of 4, 49 151: 5 of 37, 49 152: 0 of 20, 65 536: 6 of 34, C4 16 384: 0 of 11; the same in both
# finishing modes)
MAX_FLIPPED = {("c2", 12289): 2, ("c2", 16384): 2, ("c2", 49151): 7, ("c2", 49152): 2, ("c2", 65536): 8,
               ("c4", 16384): 2}

_REF = {}


def _inputs(name, B):
    cfg = dict(CONFIGS[name], B=B, seed=CONFIGS[name]["seed"] + B)
    return cfg, cases.make_inputs(cfg)


def _reference(name, B):
    """float64 (y, loss, grads, alts) of one (config, B), computed once and shared by the finishing modes."""
    if (name, B) not in _REF:
        cfg, (X, coords, t, y) = _inputs(name, B)
        params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
        _REF[(name, B)] = torch_f64.train_step_grads(X, coords, t, y, params, cfg, device=T.dev(), chunk=4096,
                                                     kink_tol=KINK_TOL)
    return _REF[(name, B)]


def _views(eng, m, buf):
    """{state_dict key: float64 array in the oracle's layout} of one of the engine's flat buffers (dW0 and W0 are
    stored transposed)."""
    by = {n: (o, k) for n, o, k in eng.offsets}
    out = {}
    for k, p in m.named_parameters():
        o, n = by[k]
        a = buf[o:o + n].double().cpu().numpy()
        out[k] = a.reshape(p.shape[1], p.shape[0]).T if k == "mlp.0.weight" else a.reshape(p.shape)
    return out


@pytest.mark.parametrize("name,B,fin", [("c2", 12289, None), ("c2", 16384, None), ("c2", 49151, None),
                                        ("c2", 49151, 2), ("c2", 49152, None), ("c2", 65536, None),
                                        ("c2", 65536, 1), ("c4", 16384, None)])
def test_large_batch_step_against_float64(name, B, fin, monkeypatch):
    from stnf.engine import TrainStep
    if any(os.environ.get(k) for k in ("STDADK_NO_DW_ALL", "STDADK_NO_FUSED_TAIL")):
        pytest.skip("the merged weight-gradient launch is switched off")
    if fin is None:
        monkeypatch.delenv("STDADK_DW_FIN", raising=False)
    else:
        monkeypatch.setenv("STDADK_DW_FIN", str(fin))
    cfg, (X, coords, t, y) = _inputs(name, B)
    yo, lo, go, alts = _reference(name, B)
    ref_norm = float(np.sqrt(sum(float((g * g).sum()) for g in go.values())))
    o = cases.OPT
    clip = 0.5 * ref_norm                                    # clipping active
    d = T.dev()
    m = T.build_model(cfg)
    m.force_window_path = False                              # the library's own choice, as in bench.py
    m.train()
    eng = TrainStep(m, lr=o["lr"], weight_decay=o["weight_decay"], betas=o["betas"], eps=R2._DP_EPS,
                    grad_clip=clip, ema_decay=o["ema_decay"], max_batch=B)
    assert eng.uses_window and eng._whole_step
    eng.step(None, *(torch.from_numpy(a).to(d) for a in (coords, t, y)))
    loss = eng.mean_loss()
    assert eng.step_dev.item() == 1
    assert abs(loss - lo) <= TOL * lo, (loss, lo)

    got = _views(eng, m, eng.grad)
    flipped, adj = orc.fit_kink_sides(got, go, alts)
    errs = {k: T.rel_l2(got[k], adj[k]) for k in got}
    worst = max(errs.values())
    print(f"{name} B={B} fin={fin}: loss rel {abs(loss - lo) / lo:.2e}; {len(alts)} units within {KINK_TOL} of a "
          f"kink, flipped {len(flipped)}: {flipped}; worst gradient rel-L2 {worst:.2e} "
          f"({max(errs, key=errs.get)})")
    assert len(flipped) <= MAX_FLIPPED[(name, B)], flipped
    for k, e in errs.items():
        assert e <= TOL, (k, e)
    # knots no row reaches: exactly zero dW0 columns in both (the fp32 kernel may flush a float64 ~1e-40 to zero)
    zk = np.abs(got["mlp.0.weight"]).sum(0) == 0
    zo = np.abs(go["mlp.0.weight"]).sum(0) == 0
    assert zo.any() or name == "c2"
    assert np.all(zk[zo])
    assert np.abs(go["mlp.0.weight"][:, zk & ~zo]).max(initial=0.0) <= 1e-25
    if name == "c4":
        return

    # one clipped AdamW + EMA step in float64 on the adjusted gradients
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    mm = {k: np.zeros_like(v) for k, v in params.items()}
    vv = {k: np.zeros_like(v) for k, v in params.items()}
    sh = {k: v.copy() for k, v in params.items()}
    coef = orc.adamw_ema_step(params, adj, mm, vv, sh, 1, o["lr"], o["weight_decay"], o["betas"], R2._DP_EPS, clip,
                              o["ema_decay"])
    assert coef < 0.6
    p_got, e_got = _views(eng, m, eng.flat), _views(eng, m, eng.ema)
    for k in params:
        assert T.rel_l2(p_got[k], params[k]) <= TOL, (k, T.rel_l2(p_got[k], params[k]))
        assert T.rel_l2(e_got[k], sh[k]) <= TOL, (k, T.rel_l2(e_got[k], sh[k]))


# ------------------------------------------------------------------ next-batch planning at the edge
def _state(eng):
    torch.cuda.synchronize()
    return [x.clone() for x in (eng.flat, eng.m, eng.v, eng.ema, eng.step_dev, eng.loss_sum)]


def _engine(cfg, B):
    from stnf.engine import TrainStep
    m = T.build_model(cfg).train()
    return TrainStep(m, lr=1e-3, grad_clip=0.5, ema_decay=0.99, max_batch=B, seed=5)


def _edge_data(n):
    cfg = dict(cases.MODEL_CASES["c2_b257"], B=n, seed=41)
    d = T.dev()
    _, coords, t, y = cases.make_inputs(cfg)
    coords, t, y = (torch.from_numpy(a).to(d) for a in (coords, t, y))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(d)
    return cfg, coords, t.view(-1), y, perm


def test_engine_refuses_next_batch_larger_than_max_batch():
    """max_batch 4096 and a next batch of 8 000 rows: the call raises before anything of the step is enqueued
    (parameters, moments, EMA, step counter and loss sum bit-identical), and the following step equals one taken
    without the failed call."""
    cfg, coords, t, y, perm = _edge_data(16384)
    a, b, big = perm[:4096], perm[4096:8192], perm[8192:16192]
    assert big.numel() == 8000
    eng, ref = _engine(cfg, 4096), _engine(cfg, 4096)
    for e in (eng, ref):
        e.step_indexed(coords, t, y, a)
    before = _state(eng)
    with pytest.raises(RuntimeError, match="max_batch"):
        eng.step_indexed(coords, t, y, b, next_idx=big)
    after = _state(eng)
    for x0, x1 in zip(before, after):
        assert torch.equal(x0, x1)
    for e in (eng, ref):
        e.step_indexed(coords, t, y, b)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat, ref.flat) and torch.equal(eng.ema, ref.ema)
    assert int(eng.step_dev.item()) == int(ref.step_dev.item()) == 2
    l_got, l_ref = eng.mean_loss(), ref.mean_loss()
    assert abs(l_got - l_ref) <= 1e-6 * l_ref


def test_one_call_step_with_unplannable_next_batch_changes_nothing():
    """stdadk_train_step_next_f32 with a next workspace too small for the next batch: the error is raised, the
    step's state is bit-identical after a synchronise, and a following normal step equals one taken without the
    failed call."""
    from stnf import _native as N
    from stnf import distributed as D
    cfg, coords, t, y, perm = _edge_data(8192)
    a, b = perm[:4096], perm[4096:]
    eng, ref = _engine(cfg, 4096), _engine(cfg, 4096)
    for e in (eng, ref):
        e.step_indexed(coords, t, y, a)
    torch.cuda.synchronize()
    assert eng._optim is not None and eng._whole_step
    before = _state(eng)
    st = eng.state
    small = torch.empty(1024, device=T.dev())
    with pytest.raises(RuntimeError):
        N.train_step_next(st.basis, st.desc, st.params, eng.grads_t, coords, t, None, y, b,
                          D.grad_scale(b.numel(), 1), eng.loss_sum, eng.ws, st.flags, eng._optim, a, small,
                          seed=eng.seed, loss_desc=eng._loss_desc(1), sparsity_desc=eng._sparsity)
    after = _state(eng)
    for x0, x1 in zip(before, after):
        assert torch.equal(x0, x1)
    for e in (eng, ref):
        e.step_indexed(coords, t, y, b)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat, ref.flat) and torch.equal(eng.ema, ref.ema)
    assert int(eng.step_dev.item()) == int(ref.step_dev.item()) == 2
    l_got, l_ref = eng.mean_loss(), ref.mean_loss()
    assert abs(l_got - l_ref) <= 1e-6 * l_ref
