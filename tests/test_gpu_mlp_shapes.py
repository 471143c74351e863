"""The fused MLP tail (csrc/tail_body.h: every hidden layer after the first, the head, the loss and the backward data
path), the dense layer 0 inside the tail launch and the per-layer fallback of mlp.hip against the float64 oracle at
the widths, depths and heads of tests/golden/shape_cases.py -- ragged last K chunks in both weight layouts, layers
in which most waves have no N tile, depth 1 and depth 8, heads of 2 / 4 / 8 outputs, feature widths at the edges of
the dense layer 0 (256 / 257 / 512 / 513) and widths the tail refuses.  The window-vs-materialised comparisons of
test_gpu_parity run the SAME tail kernels on both sides, so a wrong product there cancels; here nothing does.

Tolerances: the project's 1e-5 (test_gpu_parity, test_gpu_large_batch) -- y max-abs against max(1, max|y|), loss
relative, every gradient tensor rel-L2 after the units the oracle puts within 1e-6 of a ReLU kink may sit on either
side (orc.fit_kink_sides; at most two such units per case, tests/test_shape_cases_cpu.py).  bf16 operands: against
the emulation of test_gpu_bf16 with that module's bounds.  Every test prints what it achieved.
"""
import numpy as np
import pytest
import torch

from golden import cases
from golden import shape_cases as SC
from oracle import stdadk_oracle as orc

import test_gpu_bf16 as BF
import test_gpu_parity as T
import test_gpu_round2 as R2
from test_gpu_large_batch import _views

pytestmark = pytest.mark.gpu
TOL = 1e-5
KINK_TOL = 1e-6

_REF = {}


def _reference(name, B=None):
    """(cfg, inputs, float64 y / loss / grads / near-kink alternatives) of one case, computed once and shared."""
    key = (name, B or SC.SHAPE_CASES[name]["B"])
    if key not in _REF:
        cfg = SC.config(name, B)
        inp = SC.make_inputs(cfg)
        params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
        _REF[key] = (cfg, inp) + tuple(orc.train_step_grads(*inp, params, cfg, kink_tol=KINK_TOL))
    return _REF[key]


def _dev_inputs(cfg, inp):
    X, coords, t, y = (torch.from_numpy(a).to(T.dev()) for a in inp)
    return (X if cfg["p"] else None), coords, t, y


def _check_grads(label, got, go, alts, max_alts=2):
    flipped, adj = orc.fit_kink_sides(got, go, alts)
    errs = {k: T.rel_l2(got[k], adj[k]) for k in go}
    worst = max(errs, key=errs.get)
    print(f"{label}: {len(alts)} units within {KINK_TOL} of a kink, flipped {len(flipped)}: {flipped}; worst gradient "
          f"rel-L2 {errs[worst]:.2e} ({worst})")
    assert len(flipped) <= len(alts) <= max_alts, (flipped, len(alts))
    for k, e in errs.items():
        assert e <= TOL, (k, e)
    return adj


# ------------------------------------------------------------------ a. module forward / backward
A_PARAMS = [(n, "auto") for n in SC.SHAPE_CASES] + [(n, "dense") for n in SC.WINDOW_CASES]


@pytest.mark.parametrize("name,path", A_PARAMS)
def test_module_forward_backward_against_float64(name, path):
    from stnf import _native as N
    cfg, inp, yo, lo, go, alts = _reference(name)
    d = T.dev()
    m = T.build_model(cfg)
    m.force_dense_path = path == "dense"
    st = m._step_state(d, force_dense=m.force_dense_path)
    assert N.step_uses_window(st.basis, st.desc, st.flags) == (path == "auto" and name in SC.WINDOW_CASES)
    m.train()
    X, coords, t, y = _dev_inputs(cfg, inp)
    yp = m(X, coords, t)
    assert yp.shape == (cfg["B"], cfg["output_dim"])
    loss = torch.nn.MSELoss()(yp, y)
    loss.backward()
    err_y = np.abs(yp.detach().cpu().numpy() - yo).max() / max(1.0, float(np.abs(yo).max()))
    err_l = abs(loss.item() - lo) / lo
    print(f"{name} [{path}]: y max-abs {err_y:.2e} (of max(1, max|y|)), loss rel {err_l:.2e}")
    assert err_y <= TOL, err_y
    assert err_l <= TOL, err_l
    got = {}
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        got[k] = p.grad.cpu().numpy().astype(np.float64)
    assert set(got) == set(go)
    _check_grads(f"{name} [{path}]", got, go, alts)


# ------------------------------------------------------------------ b. one TrainStep.step
B_PARAMS = [(n, 300) for n in SC.WINDOW_CASES] + [(n, SC.BIG_B) for n in SC.BIG_CASES] \
    + [("d_D256", 300), ("d_D512", 300), ("g_h320_72_q3", 300)] \
    + [(n, B) for B in (SC.ROWS32_B, SC.ROWS64_B) for n in SC.BIG_CASES]


@pytest.mark.parametrize("name,B", B_PARAMS)
def test_train_step_against_float64(name, B):
    """TrainStep.step, the path bench.py times: gradients, then the clipped AdamW + EMA step (clipping active at half
    the reference norm) against the float64 optimiser on the kink-adjusted gradients.  Window cases at 300 rows run the
    one-launch step kernel (fused_step.hip); at 4 097 rows, the first size past it, the separate window and tail
    kernels with a ragged last tile of one row (no bound on the number of near-kink units there: fourteen times the
    rows); at 8 161 and 16 321 rows the same kernels with 32- and 64-row tiles (shape_cases.ROWS32_B / ROWS64_B), whose
    rolled K loop with a ragged last chunk no other test reaches."""
    from stnf.engine import TrainStep
    cfg, inp, yo, lo, go, alts = _reference(name, B)
    ref_norm = float(np.sqrt(sum(float((g * g).sum()) for g in go.values())))
    o = cases.OPT
    clip = 0.5 * ref_norm
    m = T.build_model(cfg)
    m.train()
    eng = TrainStep(m, lr=o["lr"], weight_decay=o["weight_decay"], betas=o["betas"], eps=R2._DP_EPS, grad_clip=clip,
                    ema_decay=o["ema_decay"], max_batch=B)
    assert eng.uses_window == (name in SC.WINDOW_CASES) and eng._whole_step
    X, coords, t, y = _dev_inputs(cfg, inp)
    eng.step(X, coords, t, y)
    loss = eng.mean_loss()
    assert eng.step_dev.item() == 1
    print(f"{name} B={B}: loss rel {abs(loss - lo) / lo:.2e}")
    assert abs(loss - lo) <= TOL * lo, (loss, lo)
    got = _views(eng, m, eng.grad)
    adj = _check_grads(f"{name} B={B}", got, go, alts, max_alts=2 if B == 300 else len(alts))

    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    mm = {k: np.zeros_like(v) for k, v in params.items()}
    vv = {k: np.zeros_like(v) for k, v in params.items()}
    sh = {k: v.copy() for k, v in params.items()}
    coef = orc.adamw_ema_step(params, adj, mm, vv, sh, 1, o["lr"], o["weight_decay"], o["betas"], R2._DP_EPS, clip,
                              o["ema_decay"])
    assert coef < 0.6
    p_got, e_got = _views(eng, m, eng.flat), _views(eng, m, eng.ema)
    ep = {k: T.rel_l2(p_got[k], params[k]) for k in params}
    ee = {k: T.rel_l2(e_got[k], sh[k]) for k in params}
    print(f"{name} B={B}: after the step, parameters worst rel-L2 {max(ep.values()):.2e} ({max(ep, key=ep.get)}), EMA "
          f"{max(ee.values()):.2e}")
    for k in params:
        assert ep[k] <= TOL, (k, ep[k])
        assert ee[k] <= TOL, (k, ee[k])


# ------------------------------------------------------------------ c. which path ran
def _step_launches(name, B=None):
    from stnf import _native as N
    from stnf.engine import TrainStep
    cfg, inp = _reference(name, B)[:2]
    m = T.build_model(cfg)
    m.train()
    eng = TrainStep(m, lr=1e-3, grad_clip=0.5, ema_decay=0.99, max_batch=cfg["B"])
    args = _dev_inputs(cfg, inp)
    eng.step(*args)                      # first call: one-time attribute calls, workspace carving
    torch.cuda.synchronize()
    N.profile_enable(True)
    try:
        eng.step(*args)
        names = [k for k, _ in N.profile_collect()]
    finally:
        N.profile_enable(False)
    print(f"{name} B={cfg['B']}: {names}")
    return names


def _has(names, part):
    return any(part in n for n in names)


@pytest.mark.parametrize("name,B", [("w_k48_q2", None), ("w_depth8_q8", None), ("w_k80_k176_noln", SC.BIG_B),
                                    ("d_D256", None), ("d_D512", None), ("d_D513", None), ("g_h40_24", None),
                                    ("g_h320_72_q3", None)])
def test_which_kernels_a_step_launches(name, B):
    """The library's own launch record of one step per family: the shapes above are worth their tests only while they
    reach the kernels they are named after, so a path that changes silently fails here."""
    names = _step_launches(name, B)
    assert _has(names, "adamw_ema_kernel") or _has(names, "adamw_bin_kernel"), names
    if name in SC.WINDOW_CASES and B is None:
        # one launch from the raw observations to the activation gradients
        assert "l1_tail_kernel" in names, names
        assert not _has(names, "l1_window_fwd_kernel") and not _has(names, "tail_fwd"), names
    elif name in SC.WINDOW_CASES:
        assert "l1_window_fwd_kernel" in names and "tail_fwd_bwd_kernel" in names, names
        assert not _has(names, "l1_tail_kernel"), names
    elif name == "d_D513":
        # layer 0 outside the launch: feature build + GEMM + its LayerNorm / ReLU kernel, then the tail
        assert _has(names, "rbf_build_kernel") and _has(names, "ln_relu_fwd_kernel"), names
        assert "tail_fwd_bwd_kernel" in names and not _has(names, "dense0"), names
    elif name in SC.DENSE0_CASES:
        assert "tail_fwd_bwd_kernel<dense0>" in names, names
        assert not _has(names, "rbf_build") and not _has(names, "ln_relu_fwd_kernel"), names
    else:
        assert not _has(names, "tail"), names
        assert _has(names, "rbf_build_kernel") and _has(names, "ln_relu_fwd_kernel") and _has(names, "ln_relu_bwd_kernel"), names
        assert _has(names, "head_bwd_kernel") or _has(names, "gemm"), names


# ------------------------------------------------------------------ d. forward only
@pytest.mark.parametrize("name", list(SC.SHAPE_CASES))
def test_predictor_against_float64(name):
    """Predictor.predict (eval-mode launches: no saved tensors, no loss).  It takes no covariates by design: the two
    p = 1 cases assert that refusal and check the module's eval forward instead."""
    from stnf.engine import Predictor
    cfg, inp, yo = _reference(name)[:3]
    m = T.build_model(cfg)
    m.eval()
    X, coords, t, _ = _dev_inputs(cfg, inp)
    pr = Predictor(m, chunk=4096)
    if cfg["p"]:
        with pytest.raises(RuntimeError, match=r"covariates \(p>0\) are not wired"):
            pr.predict(coords, t)
        with torch.no_grad():
            got = m(X, coords, t)
    else:
        got = pr.predict(coords, t)
    assert got.shape == yo.shape
    err = np.abs(got.cpu().numpy() - yo).max() / max(1.0, float(np.abs(yo).max()))
    print(f"{name}: forward-only y max-abs {err:.2e} (of max(1, max|y|))")
    assert err <= TOL, err


@pytest.mark.parametrize("name", ["w_k48_q2", "d_D257_depth1", "d_D256"])
def test_predict_grid_against_float64(name):
    """Site x time grid, S = 67 sites x T = 3 times: the tail launch starts from the two halves of layer 0's
    pre-activation (TailDense0.on == 2) -- on the window path and (d_D256) on the materialising one.  With covariates
    the grid is refused like predict()."""
    from stnf.engine import Predictor
    cfg = SC.config(name)
    S, Tn = 67, 3
    rs = np.random.RandomState(cfg["seed"] + 500)
    coords = rs.uniform(-0.05, 1.05, (S, 2)).astype(np.float32)
    tv = (np.arange(Tn, dtype=np.float32) / np.float32(Tn - 1)).astype(np.float32)
    d = T.dev()
    m = T.build_model(cfg)
    m.eval()
    pr = Predictor(m, chunk=4096)
    if cfg["p"]:
        with pytest.raises(RuntimeError, match=r"covariates \(p>0\) are not wired"):
            pr.predict_grid(torch.from_numpy(coords).to(d), torch.from_numpy(tv).to(d))
        return
    got = pr.predict_grid(torch.from_numpy(coords).to(d), torch.from_numpy(tv).to(d))
    assert got.shape == (Tn, S, cfg["output_dim"])
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    yo = orc.model_forward(None, np.tile(coords, (Tn, 1)), np.repeat(tv, S).reshape(-1, 1), params, cfg)[0]
    yo = yo.reshape(Tn, S, cfg["output_dim"])
    err = np.abs(got.cpu().numpy() - yo).max() / max(1.0, float(np.abs(yo).max()))
    print(f"{name}: {Tn} x {S} grid y max-abs {err:.2e} (of max(1, max|y|))")
    assert err <= TOL, err


# ------------------------------------------------------------------ e. bf16 operands
E_PARAMS = [pytest.param(n, None, id=n) for n in ["w_k48_q2", "w_k80_k176_noln", "w_narrow_wide_q4", "d_D256"]] \
    + [pytest.param("w_k80_k176_noln", B, id=f"w_k80_k176_noln-{B}") for B in (SC.ROWS32_B, SC.ROWS64_B)]


@pytest.mark.parametrize("name,B", E_PARAMS)
def test_bf16_operands_against_emulation(name, B):
    """K % 64 in {16, 32, 48} under bf16 operands (64-deep chunks: a piece beyond K meets zeros in the A image) against
    the float64 emulation of exactly that arithmetic (test_gpu_bf16.emulate), with that module's bounds: rounding flips
    stay below them, a wrong k mapping or a missing product shows at O(1).  The two large batches run the 32- and
    64-row tiles."""
    cfg, inp = _reference(name, B)[:2]
    m = T.build_model(cfg)
    m.compute_dtype = "bf16"
    m.train()
    X, coords, t, y = _dev_inputs(cfg, inp)
    yp = m(X, coords, t)
    loss = torch.nn.MSELoss()(yp, y)
    loss.backward()
    ye, le, ge = BF.emulate(BF.features64(cfg, m, *inp[:3]), cases.make_state(cfg), cfg, inp[3], BF.DW_BF)
    emu_y = np.abs(yp.detach().cpu().numpy() - ye).max() / max(1.0, float(np.abs(ye).max()))
    emu_l = abs(loss.item() - le) / le
    emu_g = {k: T.rel_l2(p.grad.cpu().numpy(), ge[k]) for k, p in m.named_parameters()}
    worst = max(emu_g, key=emu_g.get)
    print(f"{name} B={cfg['B']} bf16 vs emulation: y {emu_y:.2e}, loss {emu_l:.2e}, gradients worst rel-L2 {emu_g[worst]:.2e} ({worst})")
    assert emu_y <= BF.EMU_Y and emu_l <= BF.EMU_LOSS
    for k, e in emu_g.items():
        assert e <= BF.EMU_GRAD, (k, e)
