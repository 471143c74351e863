"""The one-call training step of models with the delta head: TrainStep(fused_delta_step=True) ->
stdadk_train_step_delta_f32, fixed knots (one AdamW group) or learnable knots (two).  The derived output layer is the
call's first launch; the head's fold with P_nc(delta) is ONE workgroup of the step's finishing launch
(step_finish_kernel), which also leaves the one clip-norm partial of the delta rows.

Against the float64 goldens of the split path's own tests, against the split path itself (bit for bit with clipping
off: every route, every finishing mode, bf16, last-hidden widths around the workgroup size), the clip norm against the
gradient it is the norm of, both branches and the tie of P_nc(delta), the next batch, graph replay, the non-finite
guard, a refused call, the launch names and train_model."""
import json
import math
import os

import numpy as np
import pytest
import torch

from golden import cases
from oracle import stdadk_oracle as orc

import test_gpu_parity as T

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _state(eng):
    torch.cuda.synchronize()
    return dict(flat=eng.flat.clone(), m=eng.m.clone(), v=eng.v.clone(), ema=eng.ema.clone(), grad=eng.grad.clone(),
                step=eng.step_dev.clone(), dWo=eng.d_head[0].clone(), dbo=eng.d_head[1].clone())


def _assert_same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, (a[k] != b[k]).sum().item())


def _golden_engine(name, fused, dense, **kw):
    """The engine of test_gpu_parity.test_quantile_engine_steps_match_reference on a fixed-knot delta case."""
    from stnf.engine import TrainStep
    m, cfg, lc = T.build_quantile_model(name)
    assert cfg["delta"]
    o = cases.OPT
    m.train()
    kw.setdefault("grad_clip", o["grad_clip"])
    eng = TrainStep(m, lr=o["lr"], weight_decay=o["weight_decay"], betas=o["betas"], eps=o["eps"],
                    ema_decay=o["ema_decay"], max_batch=cfg["B"], force_dense=dense, loss="pinball",
                    quantile_levels=lc["taus"], non_crossing_lambda=lc["nc_lambda"], fused_delta_step=fused, **kw)
    assert bool(eng._delta_step) == bool(fused) and not eng._whole_step and not eng._knot_step
    X, coords, t, y = (torch.from_numpy(a).to(T.dev()) for a in cases.make_inputs(cfg))
    return eng, m, cfg, lc, (X if cfg["p"] else None, coords, t, y)


# ------------------------------------------------------------------------------------------ 1. fixed knots, float64
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", ["tiny9_delta5", "default227_delta5"])
def test_fixed_knot_fused_steps_match_reference(name, dense):
    """OPT['steps'] one-call steps against the goldens and at the tolerances of
    test_gpu_parity.test_quantile_engine_steps_match_reference: 1e-4 on losses, parameters and EMA."""
    eng, m, cfg, lc, (X, coords, t, y) = _golden_engine(name, True, dense)
    g = T.load(name)
    # (the window kernels take first hidden widths of 128 / 256: tiny9's 32 runs the materialising route either way)
    assert eng.uses_window == (not dense and cfg["hidden_dims"][0] in (128, 256))
    losses = []
    for _ in range(cases.OPT["steps"]):
        eng.step(X, coords, t, y)
        losses.append(eng.mean_loss())
    ref = g["opt_losses64"]
    print(name, dense, "window" if eng.uses_window else "materialising", "losses", losses, "ref", list(ref))
    assert np.abs(np.array(losses) - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), (losses, ref)
    assert int(eng.step_dev.item()) == cases.OPT["steps"]
    for k, p in m.named_parameters():
        T.check_vs_digest(p.detach().cpu().numpy(), g, "p", k, cfg["seed"] + 7, tol=1e-4)
    eng.swap_in_ema()
    for k, p in m.named_parameters():
        T.check_vs_digest(p.detach().cpu().numpy(), g, "ema", k, cfg["seed"] + 7, tol=1e-4)
    eng.swap_in_ema()


# ------------------------------------------------------------------------------------------ 2. learnable knots, float64
def _build_learn_delta_model(name):
    """test_gpu_parity.build_learn_model for a DELTA_LEARN_CASES entry: the case's knots, trunk and head."""
    from golden import delta_learn_cases as dl
    from stnf.models import STInterpMLP
    cfg, kn, lc = dl.cfg_of(name)
    g = T.load(name)
    m = STInterpMLP(p=cfg["p"], k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=cfg["k_temporal_centers"],
                    hidden_dims=cfg["hidden_dims"], dropout=0.0, layernorm=cfg["layernorm"], spatial_learnable=True,
                    spatial_basis_function=cfg["basis"], output_dim=cfg["output_dim"], use_delta_reparameterization=True,
                    gradient_damping=kn.get("gradient_damping", False), damping_threshold=kn.get("damping_threshold", 0.3),
                    damping_strength=kn.get("damping_strength", 1.0))
    sb = m.spatial_basis
    dc, _ = cases.knot_perturbation(cfg)
    # the grid knots are bit-identical with the reference's before the perturbation
    assert np.array_equal((sb.centers.detach().numpy() + dc).astype(np.float32), g["in_centers"])
    st = dl.make_state(cfg)
    names = [k for k, _ in m.named_parameters()]
    assert names[:2] == ["spatial_basis.centers", "spatial_basis.log_bandwidths"] and names[2:] == list(st.keys())
    with torch.no_grad():
        sb.centers.copy_(torch.from_numpy(g["in_centers"]))
        sb.log_bandwidths.copy_(torch.from_numpy(g["in_log_bw"]))
        for k, p in list(m.named_parameters())[2:]:
            p.copy_(torch.from_numpy(st[k].copy()))
    m.force_window_path = True
    return m.to(T.dev()), cfg, kn, lc, g


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["default227_learn_delta5", "c2_b257_learn_delta5"])
def test_learnable_steps_match_reference(name, fused):
    """OPT['steps'] steps of the DA-STDK row (learnable knots + delta head + P_nc(delta), lambda = 1) against the float64
    goldens, fused and split (the default, the parent's path: the bound is not fitted to the new code).

    Bound per tensor: the project's own for learnable steps (test_gpu_parity.test_learnable_engine_steps_match_reference:
    5 TOL on the losses, 2e-4 on parameters and EMA); where tests/golden/delta_learn_achieved.json shows the reference's
    own float32 run deviating from its float64 run by more than half of that, twice the reference's deviation (the
    kernels sum in another order than the reference's BLAS, both in float32)."""
    from golden import delta_learn_cases as dl
    from stnf.engine import TrainStep
    m, cfg, kn, lc, g = _build_learn_delta_model(name)
    with open(os.path.join(GOLD, dl.ACHIEVED)) as f:
        ach = json.load(f)[name]
    o = cases.OPT
    m.train()
    eng = TrainStep(m, lr=o["lr"], weight_decay=o["weight_decay"], betas=o["betas"], eps=o["eps"],
                    grad_clip=o["grad_clip"], ema_decay=o["ema_decay"], max_batch=cfg["B"],
                    basis_lr_ratio=cases.BASIS_LR_RATIO, basis_clip_ratio=cases.BASIS_CLIP_RATIO,
                    domain_penalty_weight=kn.get("domain_penalty_weight", 0.0),
                    movement_penalty_weight=kn.get("movement_penalty_weight", 0.0), loss="pinball",
                    quantile_levels=lc["taus"], non_crossing_lambda=lc["nc_lambda"], fused_delta_step=fused)
    assert bool(eng._delta_step) == fused and eng.learnable and eng.uses_window
    X, coords, t, y = (torch.from_numpy(a).to(T.dev()) for a in cases.make_inputs(cfg))
    losses = []
    for _ in range(o["steps"]):
        eng.step(None, coords, t, y)
        losses.append(eng.mean_loss())
    ref = g["opt_losses64"]
    scale = max(1.0, np.abs(ref).max())

    def bound(base, achieved):
        return base if achieved <= base / 2 else 2 * achieved
    ltol = bound(5 * T.TOL, ach["losses_maxabs"] / scale)
    print(name, "fused" if fused else "split", "losses", losses, "ref", list(ref), "tol", ltol)
    assert np.abs(np.array(losses) - ref).max() <= ltol * scale, (losses, ref)
    assert int(eng.step_dev.item()) == o["steps"]
    for prefix in ("p", "ema"):
        if prefix == "ema":
            eng.swap_in_ema()
        for k, p in m.named_parameters():
            tol = bound(2e-4, ach[prefix][k])
            err = T.check_vs_digest(p.detach().cpu().numpy(), g, prefix, k, cfg["seed"] + 7, tol=tol)
            if tol != 2e-4 or err > 1e-4:
                print(" ", prefix, k, "err", err, "tol", tol, "reference f32", ach[prefix][k])
    eng.swap_in_ema()


# ------------------------------------------------------------------------------------------ 3. against the split path
def _model(hidden, Q=5, learn=False, window=True, knots=(25, 81), seed=3, delta_scale=1.0):
    """A small delta model; the delta rows are scaled up from their N(0, 0.01) start so that both branches of P_nc(delta)
    occur among the rows."""
    from stnf.models import STInterpMLP
    torch.manual_seed(seed)
    m = STInterpMLP(p=0, k_spatial_centers=list(knots), k_temporal_centers=[10, 15], hidden_dims=list(hidden),
                    dropout=0.1, layernorm=True, output_dim=Q, use_delta_reparameterization=True,
                    spatial_learnable=learn, gradient_damping=learn, damping_threshold=0.0, damping_strength=5.0)
    with torch.no_grad():
        for p in m.delta_params:
            p.mul_(delta_scale)
    m.force_window_path = bool(window)
    return m.to(T.dev()).train()


def _data(n, seed=9):
    rs = np.random.RandomState(seed)
    d = T.dev()
    return (torch.from_numpy(rs.uniform(0, 1, (n, 2)).astype(np.float32)).to(d),
            torch.from_numpy(rs.uniform(0, 1, (n,)).astype(np.float32)).to(d),
            torch.from_numpy(rs.standard_normal((n, 1)).astype(np.float32)).to(d))


def _engine(m, fused, B, taus=None, **kw):
    from stnf.engine import TrainStep
    Q = m.output_dim
    kw.setdefault("grad_clip", 0)
    kw.setdefault("lr", 1e-3)
    eng = TrainStep(m, ema_decay=0.99, max_batch=B, loss="pinball",
                    quantile_levels=taus or list(np.linspace(0.05, 0.95, Q)), non_crossing_lambda=1.0,
                    domain_penalty_weight=0.01 if m.spatial_basis.learnable else 0.0, seed=4,
                    fused_delta_step=fused, **kw)
    assert bool(eng._delta_step) == bool(fused)
    return eng


def _fused_vs_split(make_model, B, steps=3, **kw):
    coords, t, y = _data(B)
    res = {}
    for fused in (True, False):
        m = make_model()
        eng = _engine(m, fused, B, **kw)
        for _ in range(steps):
            eng.step(None, coords, t, y)
        res[fused] = _state(eng)
        res[fused]["loss"] = eng.mean_loss()
        if eng._shadow_buf is not None:
            res[fused]["bf16"] = eng._shadow_buf.clone()
        assert int(res[fused]["step"].item()) == steps and torch.isfinite(res[fused]["flat"]).all()
        res[fused]["window"] = eng.uses_window
        del eng, m
    la, lb = res[True].pop("loss"), res[False].pop("loss")
    wa, wb = res[True].pop("window"), res[False].pop("window")
    assert wa == wb
    # (the penalty and the data term are added into the accumulator in another order)
    assert abs(la - lb) <= 1e-6 * max(1.0, abs(lb)), (la, lb)
    _assert_same_bits(res[True], res[False], "fused vs split")
    assert res[True]["dWo"].abs().max() > 0 and res[True]["grad"].abs().max() > 0
    return wa


ROUTES = {
    "fixed_window": dict(hidden=(128, 64), learn=False, window=True),
    "fixed_materialising": dict(hidden=(64, 64), learn=False, window=False),
    "fixed_packed": dict(hidden=(256, 128), learn=False, window=True),
    "learnable_materialising": dict(hidden=(64, 64), learn=True, window=False),
    "learnable_window_small": dict(hidden=(128, 64), learn=True, window=True),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_unclipped_steps_equal_the_split_path_bit_for_bit(route):
    """Clipping off: three steps leave the same bits in parameters, moments, EMA, gradient, step counter and the output
    layer's gradient scratch as the split calls (delta_head, train_fwd_bwd, delta_head_backward[, knot_backward], adamw)."""
    r = ROUTES[route]
    window = _fused_vs_split(lambda: _model(r["hidden"], learn=r["learn"], window=r["window"], delta_scale=20.0), 257)
    assert window == r["window"]


def test_learnable_c2_window_equals_the_split_path_bit_for_bit():
    """The three-level C2 grid of c2_b257_learn_delta5 (10 304 learnable knots, window route), 257 rows."""
    cfg, kn = cases.learn_cfg("c2_b257_learn")
    _fused_vs_split(lambda: _model(cfg["hidden_dims"], learn=True, window=True, knots=cfg["k_spatial_centers"],
                                   delta_scale=20.0), cfg["B"], taus=cases.TAUS5)


@pytest.mark.parametrize("learn", [False, True])
@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_finishing_modes_equal_the_split_path_bit_for_bit(mode, learn, monkeypatch):
    """STDADK_DW_FIN = 0 / 1 / 2 on the window route at 257 rows: the head workgroup runs the output layer's sums itself
    in every mode (in mode 2 the weight-gradient launch has done all the others)."""
    monkeypatch.setenv("STDADK_DW_FIN", mode)
    assert _fused_vs_split(lambda: _model((128, 64), learn=learn, window=True, delta_scale=20.0), 257)


@pytest.mark.parametrize("learn", [False, True])
def test_bf16_equals_the_split_path_bit_for_bit(learn):
    assert _fused_vs_split(lambda: _model((128, 128, 64), learn=learn, window=True, delta_scale=20.0), 257, dtype="bf16")


@pytest.mark.parametrize("Q", [2, 5, 8])
@pytest.mark.parametrize("d", [8, 16, 37, 128, 256])
def test_last_hidden_widths_equal_the_split_path_bit_for_bit(d, Q):
    """d + 1 columns against 256 threads (d = 256: 257 columns, the column loop takes a second turn), Q up to
    STDADK_MAX_Q = 8; d = 37 is a width the fused tail kernels refuse (generic kernels: the output layer's gradient is
    final before the finishing launch and the head workgroup only folds)."""
    _fused_vs_split(lambda: _model((128, d), Q=Q, window=True, delta_scale=20.0), 70, steps=2)


# ------------------------------------------------------------------------------------------ 4. the clip norm
def _check_clip_norm(eng, max_norm):
    """sum(partials the optimiser read) against sum(g^2) over the MLP range of the flat gradient, both in float64.

    Bound.  Every partial is a sum of squares, all terms >= 0, so the rounding errors add up relatively:
    partial = sum_i g_i^2 (1 + th_i), |th_i| <= gamma_d = d u / (1 - d u), u = 2^-24, d = the longest chain of roundings
    an entry passes on its way into its partial.  The three kinds of workgroup that leave partials here:
        reduce workgroup   wide job: (x^2 + y^2) + (z^2 + w^2) of the float4 = 3 (tall job: the square alone = 1)
        region workgroup   (window route, finishing mode 0) a thread's fmaf chain over its float4s: the region of
                           106 x 128 floats gives every thread at most one float4 = 4
        head workgroup     fmaf(g, g, sq) over the Q = 5 rows of the thread's columns, one column per thread at
                           d + 1 = 65 <= 256: 5
    then for each the wave's tree over 64 lanes = 6 and (w0 + w1) + (w2 + w3) over the four waves = 2.  Longest:
    5 + 6 + 2 = 13.  The partials are added here in float64 and the gradient entries read back are the very floats that
    were squared, so nothing else enters: |sum(partials) - sum(g^2)| <= gamma_13 sum(g^2)."""
    torch.cuda.synchronize()
    g = eng.grad[eng.knot_end:].double().cpu().numpy()
    parts = eng._sumsq512.double().cpu().numpy()
    u, d = 2.0 ** -24, 13
    bound = d * u / (1 - d * u)
    want, got = float((g ** 2).sum()), float(parts.sum())
    dd = eng.d_delta.double().cpu().numpy()
    head = float((eng.d_head[0].double() ** 2).sum().item() + (eng.d_head[1].double() ** 2).sum().item())
    wrong = want - float((dd ** 2).sum()) + head
    print(f"sum(partials)={got!r} sum(g^2)={want!r} rel={abs(got - want) / want:.3e} bound={bound:.3e} "
          f"with |dWo|^2+|dbo|^2 for |d_delta|^2: {wrong!r} rel={abs(got - wrong) / want:.3e}")
    assert want > max_norm ** 2, (want, max_norm)            # the clip coefficient is below 1
    assert abs(got - want) <= bound * want
    assert abs(got - wrong) > bound * want                   # teeth: the output layer's own squares would miss it
    assert (dd ** 2).sum() > 0 and head > 0


@pytest.mark.parametrize("route", ["materialising", "window_fin0"])
@pytest.mark.parametrize("learn", [False, True])
def test_clip_norm_is_the_flat_gradients(route, learn, monkeypatch):
    """The routes whose launches leave the partials in the optimiser descriptor's own buffer, where a test can read
    them: the materialising route (reduce workgroups + the head's slot) and the window route in finishing mode 0 (256
    region workgroups + reduce workgroups + the head's slot).  One step on a fresh engine: the slots behind the last one
    written are the zeros the buffer was allocated with."""
    window = route != "materialising"
    if window:
        monkeypatch.setenv("STDADK_DW_FIN", "0")
    m = _model((128, 64) if window else (64, 64), learn=learn, window=window, delta_scale=20.0, seed=11)
    coords, t, y = _data(257)
    eng = _engine(m, True, 257, grad_clip=1e-3)
    from stnf import _native as N
    N.profile_enable(True)
    try:
        eng.step(None, coords, t, y)
        names = [k for k, _ in N.profile_collect()]
    finally:
        N.profile_enable(False)
    print(names)
    assert not any("sumsq" in k for k in names), names        # the partials came out of the step's own launches
    _check_clip_norm(eng, 1e-3)


# ------------------------------------------------------------------------------------------ 5. P_nc(delta) branches
def test_both_branches_and_the_tie_of_the_penalty():
    """n3_known_answers' ka_delta (J = 0 row, tie row, clamp-boundary row) as the head of a model whose last hidden width
    is 8; one fused step with lr = 0.  The delta rows of the gradient against orc.delta_head_backward(dWo, dbo) +
    lambda * dP_nc, from the read-back scratch, within the 1e-5 of the kernel's own test; the accumulator's penalty
    share against lambda * B * Q * P."""
    g = T.load("n3_known_answers")
    delta64 = g["ka_delta"]
    Q, d1 = delta64.shape
    assert d1 == 9
    lam, B = 0.3, 70
    coords, t, y = _data(B)
    acc = {}
    for lam_run in (lam, 0.0):
        from stnf.engine import TrainStep
        m = _model((128, 8), Q=Q, window=True)
        with torch.no_grad():
            for k, p in enumerate(m.delta_params):
                p.copy_(torch.from_numpy(delta64[k]).float())
        eng = TrainStep(m, lr=0.0, grad_clip=0, ema_decay=0.99, max_batch=B, loss="pinball",
                        quantile_levels=list(np.linspace(0.05, 0.95, Q)), non_crossing_lambda=lam_run, seed=4,
                        fused_delta_step=True)
        eng.step(None, coords, t, y)
        torch.cuda.synchronize()
        acc[lam_run] = float(eng.loss_sum.item())
        if lam_run:
            dW, db = eng.d_head[0].cpu().numpy(), eng.d_head[1].cpu().numpy()
            got = eng.d_delta.cpu().numpy()
            for k, p in enumerate(m.delta_params):          # lr = 0: nothing moved
                assert np.array_equal(p.detach().cpu().numpy(), delta64[k].astype(np.float32))
    P, gP = orc.p_nc_delta(delta64.astype(np.float32))
    ref = orc.delta_head_backward(dW, db) + lam * gP
    print("max |d_delta - ref|", np.abs(got - ref).max(), "P", P, "acc", acc)
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    want = lam * B * Q * float(P)
    assert abs((acc[lam] - acc[0.0]) - want) <= 1e-5 * max(1.0, abs(acc[lam]), abs(want)), (acc, want)


# ------------------------------------------------------------------------------------------ 6. next batch
@pytest.mark.parametrize("learn", [False, True])
def test_next_batch_announced_inline_side_stream_and_not_at_all(learn):
    """step_indexed(next_idx=...) over four batches of 64 rows: the same bits with the next batch binned inside the step
    (inline_prep), on the side stream, and without announcing."""
    d = T.dev()
    n, B = 4 * 64 + 5, 64
    coords, t, y = _data(n, seed=61)
    perm = torch.randperm(n, generator=torch.Generator(device="cpu").manual_seed(3)).to(d)
    batches = [perm[i * B:(i + 1) * B] for i in range(4)]
    res = {}
    for how in ("inline", "side", "none"):
        m = _model((128, 64), learn=learn, window=True, delta_scale=20.0)
        eng = _engine(m, True, B, inline_prep=(how == "inline"))
        eng.indexed_min_batch = 0
        took = 0
        for i, idx in enumerate(batches):
            nxt = batches[i + 1] if (i + 1 < len(batches) and how != "none") else None
            eng.step_indexed(coords, t, y, idx, next_idx=nxt)
            if nxt is not None:
                assert eng._prepared is not None
                took += bool(eng._prepared.inline)
        assert took == (3 if how == "inline" else 0), (how, took)
        res[how] = _state(eng)
        assert int(res[how]["step"].item()) == 4
        del eng, m
    _assert_same_bits(res["inline"], res["side"], "inline vs side stream")
    _assert_same_bits(res["inline"], res["none"], "inline vs not announced")


# ------------------------------------------------------------------------------------------ 7. graph, 8. guard
@pytest.mark.parametrize("learn", [False, True])
def test_graph_replay_equals_eager(learn):
    coords, t, y = _data(64)
    res = []
    for graph in (False, True):
        m = _model((128, 64), learn=learn, window=True, delta_scale=20.0)
        eng = _engine(m, True, 64, use_graph=graph, grad_clip=10.0)
        for s in range(4):
            eng.step(None, coords, t, y)
        res.append(_state(eng))
        assert int(res[-1]["step"].item()) == 4
        del eng, m
    _assert_same_bits(res[0], res[1], "graph vs eager")


def test_the_guard_names_the_step_of_a_nan_target():
    d = T.dev()
    coords, t, y = _data(128)
    m = _model((128, 64), window=True)
    eng = _engine(m, True, 64)
    eng.step_indexed(coords, t, y, torch.arange(64, device=d))
    assert eng.first_nonfinite_step() is None
    bad = y.clone()
    bad[40] = float("nan")
    eng.step_indexed(coords, t, bad, torch.arange(64, device=d))           # step 2: a NaN target
    eng.step_indexed(coords, t, y, torch.arange(64, device=d) + 32)
    assert eng.first_nonfinite_step() == 2


# ------------------------------------------------------------------------------------------ 9. a refused call
def test_a_refused_call_leaves_the_state_untouched():
    coords, t, y = _data(64)
    m = _model((128, 64), window=True, delta_scale=20.0)
    eng = _engine(m, True, 64, grad_clip=1.0)
    eng.step(None, coords, t, y)
    eng.loss_sum.fill_(3.5)
    before = _state(eng)
    before["loss_sum"] = eng.loss_sum.clone()
    good = eng.d_delta
    # the same shape and row stride, but outside the gradient range [opt->g, opt->g + n)
    eng.d_delta = torch.zeros(good.shape[0], good.stride(0), device=good.device)[:, :good.shape[1]]
    with pytest.raises(RuntimeError, match="d_delta .* lies outside the gradient range"):
        eng._enqueue(None, coords, t.view(-1), y, 64, 64)
    eng.d_delta = good
    after = _state(eng)
    after["loss_sum"] = eng.loss_sum.clone()
    _assert_same_bits(before, after, "refused call")
    eng.step(None, coords, t, y)                         # and the engine steps on
    assert int(eng.step_dev.item()) == 2


# ------------------------------------------------------------------------------------------ 10. launch names
@pytest.fixture(scope="module")
def recorded():
    import test_delta_step_cpu as chains
    rec = chains.record_chains("cuda:0", only=chains.GPU_CASES)
    torch.cuda.synchronize()
    return rec


@pytest.mark.parametrize("name", ["delta/fixed_window", "delta/learn_window"])
def test_real_launches_carry_the_dry_run_names(recorded, name):
    import test_delta_step_cpu as chains
    assert name in chains.GPU_CASES
    print(name, recorded[name])
    assert recorded[name] == chains.expected_chains()[name]


# ------------------------------------------------------------------------------------------ 11. train_model
@pytest.mark.parametrize("learn", [False, True])
def test_train_model_with_the_config_key(learn):
    """Two epochs of train_model on a tiny DeviceDataset with `fused_delta_step: true` and `grad_clip: 0`: the final
    parameters have the bits of the run with the key off."""
    from stnf import training as TR
    from stnf.dataio.device_dataset import DeviceDataset
    coords, t, y = _data(160, seed=21)
    out = {}
    for key in (True, False):
        m = _model((128, 64), learn=learn, window=True, delta_scale=20.0)
        ds = DeviceDataset(coords[:128].contiguous(), t[:128].reshape(-1, 1).contiguous(), y[:128].contiguous())
        dv = DeviceDataset(coords[128:].contiguous(), t[128:].reshape(-1, 1).contiguous(), y[128:].contiguous())
        config = dict(lr=1e-3, weight_decay=1e-5, grad_clip=0, batch_size=64, epochs=2, regression_type="multi-quantile",
                      quantile_levels=cases.TAUS5, use_delta_reparameterization=True, non_crossing_lambda=1.0,
                      spatial_learnable=learn, domain_penalty_weight=0.01, dropout_seed=5, fused_delta_step=key,
                      verbose=False)
        TR.train_model(m, ds, dv, config, shuffle=False)
        torch.cuda.synchronize()
        out[key] = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()
        del m
    assert torch.equal(out[True], out[False]), (out[True] != out[False]).sum().item()
