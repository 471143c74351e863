"""The one-call training step of learnable-knot models: TrainStep(fused_knot_step=True) -> stdadk_train_step_knots_f32,
whose finishing launch (step_finish_kernel) closes the gradients of both AdamW groups and leaves both clip norms.

Against the float64 goldens of the split path's own test, against the split path itself (bit for bit where the
arithmetic is the same: clipping off), the knot group's norm against the gradient it is the norm of, every finishing
mode of the weight-gradient launch, the launch list, the next batch binned inside the weight-gradient launch, graph
replay, frozen knots, the non-finite guard, the quantile objective and bf16 operands."""
import math

import numpy as np
import pytest
import torch

from golden import cases

import test_gpu_parity as T

pytestmark = pytest.mark.gpu

KNOT_PARTS = 256          # STDADK_SUMSQ_PARTS: the knot workgroups of the finishing launch, one partial each


def _engine(name, fused, dense=False, grad_clip=None, max_batch=None, **kw):
    """The engine of test_learnable_engine_steps_match_reference on a LEARN_CASES entry, on the chosen path."""
    from stnf.engine import TrainStep
    m, cfg, kn, g = T.build_learn_model(name)
    o = cases.OPT
    m.train()
    eng = TrainStep(m, lr=o["lr"], weight_decay=o["weight_decay"], betas=o["betas"], eps=o["eps"],
                    grad_clip=o["grad_clip"] if grad_clip is None else grad_clip, ema_decay=o["ema_decay"],
                    max_batch=max_batch or cfg["B"], basis_lr_ratio=cases.BASIS_LR_RATIO,
                    basis_clip_ratio=cases.BASIS_CLIP_RATIO, domain_penalty_weight=kn.get("domain_penalty_weight", 0.0),
                    movement_penalty_weight=kn.get("movement_penalty_weight", 0.0), force_dense=dense,
                    fused_knot_step=fused, **kw)
    assert bool(eng._knot_step) == bool(fused) and not eng._whole_step
    X, coords, t, y = (torch.from_numpy(a).to(T.dev()) for a in cases.make_inputs(cfg))
    return eng, m, cfg, g, (X if cfg["p"] else None, coords, t, y)


def _state(eng):
    torch.cuda.synchronize()
    return dict(flat=eng.flat.clone(), m=eng.m.clone(), v=eng.v.clone(), ema=eng.ema.clone(), grad=eng.grad.clone(),
                step=eng.step_dev.clone())


def _assert_same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, (a[k] != b[k]).sum().item())


# ------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", list(cases.LEARN_CASES))
def test_fused_steps_match_reference(name, dense):
    """OPT['steps'] one-call steps against the goldens and at the tolerances of
    test_gpu_parity.test_learnable_engine_steps_match_reference (5 TOL on the losses, 2e-4 on parameters and EMA)."""
    eng, m, cfg, g, (X, coords, t, y) = _engine(name, True, dense)
    assert eng._knot_step
    windowable = cfg["basis"] != "gaussian" and cfg["hidden_dims"][0] in (128, 256)
    assert eng.learnable and eng.uses_window == (windowable and not dense)
    losses = []
    for _ in range(cases.OPT["steps"]):
        eng.step(X, coords, t, y)
        losses.append(eng.mean_loss())
    ref = g["opt_losses64"]
    print(name, dense, "losses", losses, "ref", list(ref))
    assert np.abs(np.array(losses) - ref).max() <= 5 * T.TOL * max(1.0, np.abs(ref).max()), (losses, ref)
    assert int(eng.step_dev.item()) == cases.OPT["steps"]
    for k, p in m.named_parameters():
        T.check_vs_digest(p.detach().cpu().numpy(), g, "p", k, cfg["seed"] + 7, tol=2e-4)
    eng.swap_in_ema()
    for k, p in m.named_parameters():
        T.check_vs_digest(p.detach().cpu().numpy(), g, "ema", k, cfg["seed"] + 7, tol=2e-4)
    eng.swap_in_ema()


# ------------------------------------------------------------------------------------------ 2. against the split path
@pytest.mark.parametrize("name", ["c2_b257_learn", "default227_learn_gauss"])
def test_unclipped_steps_equal_the_split_path_bit_for_bit(name):
    """Clipping off: the clip coefficient is exactly 1 on both paths, every other launch and sum is the same, so three
    steps leave the same bits in the parameters, moments, EMA, gradient and step counter (window route: c2_b257_learn;
    materialising route: default227_learn_gauss)."""
    res = {}
    for fused in (True, False):
        eng, m, cfg, g, (X, coords, t, y) = _engine(name, fused, grad_clip=0)
        assert eng.uses_window == (name == "c2_b257_learn")
        for _ in range(3):
            eng.step(X, coords, t, y)
        res[fused] = _state(eng)
        assert int(res[fused]["step"].item()) == 3
        del eng, m
    _assert_same_bits(res[True], res[False], name)


# ------------------------------------------------------------------------------------------ 3. the knot group's norm
def _big_single_level_model():
    """One level of 129 x 129 = 16 641 knots = 260 tiles of 64 + 1 knot: more tiles than knot workgroups (256), so the
    workgroups stride over the tiles and the last tile is ragged."""
    from stnf.models import STInterpMLP
    torch.manual_seed(5)
    m = STInterpMLP(p=0, k_spatial_centers=[129 * 129], k_temporal_centers=[10], hidden_dims=[128, 128], dropout=0.0,
                    layernorm=True, spatial_learnable=True, gradient_damping=True, damping_threshold=0.0,
                    damping_strength=5.0)
    m.force_window_path = True
    return m.to(T.dev()).train()


def _big_engine(fused):
    from stnf.engine import TrainStep
    m = _big_single_level_model()
    eng = TrainStep(m, lr=1e-3, grad_clip=1.0, ema_decay=0.99, max_batch=300, domain_penalty_weight=0.01,
                    movement_penalty_weight=0.05, fused_knot_step=fused)
    assert eng.uses_window and bool(eng._knot_step) == fused
    rs = np.random.RandomState(77)
    d = T.dev()
    coords = torch.from_numpy(rs.uniform(-0.02, 1.02, (300, 2)).astype(np.float32)).to(d)
    t = torch.from_numpy(rs.uniform(0, 1, (300,)).astype(np.float32)).to(d)
    y = torch.from_numpy(rs.standard_normal((300, 1)).astype(np.float32)).to(d)
    return eng, m, (None, coords, t, y)


def _check_knot_norm(eng, Ks):
    """sum(partials) against sum(g^2) of the knot group's gradient, both in float64.

    Bound.  The knot workgroup's partial is a sum of the squares of the entries it wrote, all terms >= 0, so the
    rounding errors add up relatively: partial = sum_i g_i^2 (1 + th_i) with |th_i| <= gamma_d = d u / (1 - d u),
    u = 2^-24, d = the longest chain of roundings an entry passes on its way into the partial:
        1      the square
        2      (gx^2 + gy^2) + gl^2 of the knot
        T      the lane's running sum over its tiles, T = ceil(tiles / 256) tiles per lane
        6      the wave's tree over 64 lanes
        2      (w0 + w1) + (w2 + w3) over the four waves
    (a fused multiply-add only removes roundings).  The <= 256 partials are added here in float64, and the entries read
    back are the very floats that were squared, so nothing else enters: |sum(partials) - sum(g^2)| <= gamma_d sum(g^2)."""
    torch.cuda.synchronize()
    ke = eng.knot_end
    g = eng.grad[:ke].double().cpu().numpy()
    parts = eng.sumsq_basis.double().cpu().numpy()
    assert parts.shape == (KNOT_PARTS,)
    tiles = -(-Ks // 64)
    d = 1 + 2 + math.ceil(tiles / KNOT_PARTS) + 6 + 2
    u = 2.0 ** -24
    bound = d * u / (1 - d * u)
    want = float((g ** 2).sum())
    got = float(parts.sum())
    print(f"Ks={Ks} tiles={tiles} sum(partials)={got!r} sum(g^2)={want!r} rel={abs(got - want) / want:.3e} bound={bound:.3e}")
    assert want > 0 and abs(got - want) <= bound * want
    # one partial per knot workgroup, zeros behind the last one
    assert (parts[min(tiles, KNOT_PARTS):] == 0).all() and (parts >= 0).all()
    # padding of the group's gradient range (every tensor padded to a multiple of 4 floats) stays exactly zero
    used = np.zeros(ke, dtype=bool)
    for _, o, k in eng.offsets[:2]:
        used[o:o + k] = True
    assert used.sum() == 3 * Ks
    assert (g[~used] == 0).all()
    assert np.abs(g[used]).max() > 0


@pytest.mark.parametrize("name", ["tiny9_learn", "default227_learn"])
def test_knot_partials_are_the_knot_gradients_norm(name):
    """9 knots: one ragged tile (and padding behind both knot tensors); 227 = 3 x 64 + 35."""
    eng, m, cfg, g, (X, coords, t, y) = _engine(name, True)
    assert eng.basis_clip > 0
    eng.step(X, coords, t, y)
    _check_knot_norm(eng, sum(cfg["k_spatial_centers"]))


def test_knot_partials_with_more_tiles_than_workgroups():
    """16 641 knots on the window path: the tile stride and a ragged last tile; the knot gradients equal the split
    path's bit for bit (the same per-knot sums, penalties and damping, whichever kernel carries the tile)."""
    eng, m, (X, coords, t, y) = _big_engine(True)
    eng.step(X, coords, t, y)
    _check_knot_norm(eng, 129 * 129)
    gc, gl = eng.g_centers.clone(), eng.g_log_bw.clone()
    del eng, m
    ref, m2, (X, coords, t, y) = _big_engine(False)
    ref.step(X, coords, t, y)
    torch.cuda.synchronize()
    assert torch.equal(gc, ref.g_centers) and torch.equal(gl, ref.g_log_bw)
    assert gc.abs().max() > 0 and gl.abs().max() > 0


# ------------------------------------------------------------------------------------------ 4. finishing modes
@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_finishing_modes_of_the_weight_gradient_launch(mode, monkeypatch):
    """STDADK_DW_FIN = 0 / 1: the finishing launch carries the step's reduce jobs (0: the region partials in a launch
    of their own); 2: the weight-gradient launch has done the sums and the finishing launch runs with zero reduce
    workgroups.  The launch list of the first step, its loss against the golden, then -- the golden holds the
    parameters after OPT['steps'] steps, not after one -- the remaining steps and the stepped parameters and EMA,
    at the tolerances of test 1."""
    from stnf import _native as N
    monkeypatch.setenv("STDADK_DW_FIN", mode)
    eng, m, cfg, g, (X, coords, t, y) = _engine("c2_b257_learn", True)
    ref = g["opt_losses64"]
    N.profile_enable(True)
    try:
        eng.step(X, coords, t, y)
        names = [k for k, _ in N.profile_collect()]
    finally:
        N.profile_enable(False)
    losses = [eng.mean_loss()]
    print("mode", mode, names, losses, ref[0])
    assert names.count("step_finish_kernel") == 1 and names[-1] == "adamw_ema2_kernel", names
    assert ("reduce_jobs_kernel" in names) == (mode == "0"), names     # (mode 0: the 256 region workgroups alone)
    assert not any("sumsq" in k or "knot_finish" in k for k in names), names
    assert abs(losses[0] - ref[0]) <= 5 * T.TOL * max(1.0, abs(ref[0])), (losses, ref)
    for _ in range(1, cases.OPT["steps"]):
        eng.step(X, coords, t, y)
        losses.append(eng.mean_loss())
    assert np.abs(np.array(losses) - ref).max() <= 5 * T.TOL * max(1.0, np.abs(ref).max()), (mode, losses, ref)
    for k, p in m.named_parameters():
        T.check_vs_digest(p.detach().cpu().numpy(), g, "p", k, cfg["seed"] + 7, tol=2e-4)
    eng.swap_in_ema()
    for k, p in m.named_parameters():
        T.check_vs_digest(p.detach().cpu().numpy(), g, "ema", k, cfg["seed"] + 7, tol=2e-4)


# ------------------------------------------------------------------------------------------ 5. launch list
def _launches(fused):
    from stnf import _native as N
    eng, m, cfg, g, (X, coords, t, y) = _engine("c2_b257_learn", fused)
    eng.step(X, coords, t, y)
    torch.cuda.synchronize()
    N.profile_enable(True)
    try:
        eng.step(X, coords, t, y)
        names = [k for k, _ in N.profile_collect()]
    finally:
        N.profile_enable(False)
    return names


def test_launch_list_of_a_fused_and_a_split_step():
    names = _launches(True)
    print("fused", names)
    dw = [i for i, k in enumerate(names) if k.startswith("dw_all_kernel")]
    opt = [i for i, k in enumerate(names) if k.startswith("adamw_")]
    assert len(dw) == 1 and len(opt) == 1 and names[opt[0]] == "adamw_ema2_kernel" and opt[0] == len(names) - 1, names
    assert names[dw[0] + 1:opt[0]] == ["step_finish_kernel"], names
    for word in ("sumsq", "knot_finish", "reduce_jobs", "step_advance"):
        assert not any(word in k for k in names), (word, names)
    split = _launches(False)
    print("split", split)
    for word in ("sumsq2_kernel", "knot_finish_kernel", "reduce_jobs_kernel", "adamw_ema2_kernel"):
        assert word in split, (word, split)
    assert "step_finish_kernel" not in split
    assert len(split) == len(names) + 2, (names, split)


# ------------------------------------------------------------------------------------------ 6. next batch inline
def test_next_batch_is_binned_inside_the_weight_gradient_launch():
    """Four announced steps of 512 rows on the C2-sized learnable model: inline_prep=True (the library bins the next
    batch in the weight-gradient launch) against False (side stream); same bits."""
    from stnf import _native as N
    d = T.dev()
    n, B = 4 * 512 + 37, 512
    rs = np.random.RandomState(61)
    coords = torch.from_numpy(rs.uniform(0, 1, (n, 2)).astype(np.float32)).to(d)
    t = torch.from_numpy(rs.uniform(0, 1, (n,)).astype(np.float32)).to(d)
    y = torch.from_numpy(rs.standard_normal((n, 1)).astype(np.float32)).to(d)
    perm = torch.randperm(n, generator=torch.Generator(device="cpu").manual_seed(3)).to(d)
    batches = [perm[i * B:(i + 1) * B] for i in range(4)]
    res, names = {}, None
    for inline in (True, False):
        eng, m, cfg, g, _ = _engine("c2_b257_learn", True, inline_prep=inline, grad_clip=0.5, max_batch=B)
        took = 0
        for i, idx in enumerate(batches):
            nxt = batches[i + 1] if i + 1 < len(batches) else None
            if inline and i == 1:
                torch.cuda.synchronize()
                N.profile_enable(True)
            eng.step_indexed(coords, t, y, idx, next_idx=nxt)
            if inline and i == 1:
                names = [k for k, _ in N.profile_collect()]
                N.profile_enable(False)
            if nxt is not None:
                assert eng._prepared is not None
                took += bool(eng._prepared.inline)
        assert took == (3 if inline else 0)           # the library reported next_binned = 1 for every announced batch
        res[inline] = _state(eng)
        assert int(res[inline]["step"].item()) == 4
        del eng, m
    _assert_same_bits(res[True], res[False], "inline vs side stream")
    print(names)
    assert any(k.startswith("dw_all_kernel") for k in names) and "step_finish_kernel" in names, names
    assert "adamw_ema2_kernel" in names and "adamw_bin_kernel" not in names and "bin_small_kernel" not in names, names
    assert not any(k.startswith("bin_") for k in names), names     # no binning launch of its own anywhere in the step


# ------------------------------------------------------------------------------------------ 7. graph, freeze, guard
def test_graph_replay_equals_eager():
    res = []
    for graph in (False, True):
        eng, m, cfg, g, (X, coords, t, y) = _engine("default227_learn", True, use_graph=graph)
        for _ in range(3):
            eng.step(X, coords, t, y)
        res.append(_state(eng))
        assert int(res[-1]["step"].item()) == 3
        del eng, m
    _assert_same_bits(res[0], res[1], "graph vs eager")


def test_frozen_knots_do_not_move_and_the_guard_names_the_step():
    from stnf.engine import TrainStep
    d = T.dev()
    m, cfg, kn, g = T.build_learn_model("default227_learn")
    m.train()
    X, coords, t, y = (torch.from_numpy(a).to(d) for a in cases.make_inputs(cfg))
    eng = TrainStep(m, lr=1e-3, grad_clip=10.0, ema_decay=0.99, max_batch=64, domain_penalty_weight=0.01,
                    fused_knot_step=True)
    assert eng._knot_step
    c0 = m.spatial_basis.centers.detach().clone()
    b0 = m.spatial_basis.log_bandwidths.detach().clone()
    w0 = m._body[0].weight.detach().clone()
    eng.set_basis_lr(0.0)
    eng.step_indexed(coords, t, y, torch.arange(64, device=d))
    assert torch.equal(m.spatial_basis.centers.detach(), c0)              # frozen: lr 0 => no move, no decay
    assert torch.equal(m.spatial_basis.log_bandwidths.detach(), b0)
    assert not torch.equal(m._body[0].weight.detach(), w0)                # the MLP group does step
    eng.set_basis_lr(1e-3 * 0.05)
    eng.step_indexed(coords, t, y, torch.arange(64, device=d) + 16)
    assert not torch.equal(m.spatial_basis.centers.detach(), c0)
    assert eng.first_nonfinite_step() is None
    bad = y.clone()
    bad[40] = float("nan")
    eng.step_indexed(coords, t, bad, torch.arange(64, device=d))          # step 3: a NaN target
    eng.step_indexed(coords, t, y, torch.arange(64, device=d) + 32)
    assert eng.first_nonfinite_step() == 3


# ------------------------------------------------------------------------------------------ 8. quantiles, 9. bf16
def _mq5_engine(fused, dtype="f32"):
    """The shipped YAML's shape minus the delta head: 227 learnable knots, five quantile levels, non-crossing weight."""
    from stnf.engine import TrainStep
    from stnf.models import STInterpMLP
    cfg, kn = cases.learn_cfg("default227_learn")
    torch.manual_seed(8)
    m = STInterpMLP(p=0, k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=cfg["k_temporal_centers"],
                    hidden_dims=cfg["hidden_dims"], dropout=0.1, layernorm=True, spatial_learnable=True, output_dim=5,
                    gradient_damping=True, damping_threshold=0.0, damping_strength=5.0)
    m.force_window_path = True
    m = m.to(T.dev()).train()
    eng = TrainStep(m, lr=1e-3, grad_clip=0, ema_decay=0.99, max_batch=cfg["B"], loss="pinball",
                    quantile_levels=cases.TAUS5, non_crossing_weight=0.5, domain_penalty_weight=0.01, seed=4,
                    dtype=dtype, fused_knot_step=fused)
    assert eng.uses_window and bool(eng._knot_step) == fused
    X, coords, t, y = (torch.from_numpy(a).to(T.dev()) for a in cases.make_inputs(cfg))
    return eng, m, (None, coords, t, y)


def test_five_quantiles_equal_the_split_path_bit_for_bit():
    res = {}
    for fused in (True, False):
        eng, m, (X, coords, t, y) = _mq5_engine(fused)
        for _ in range(3):
            eng.step(X, coords, t, y)
        res[fused] = _state(eng)
        assert torch.isfinite(res[fused]["flat"]).all()
        del eng, m
    _assert_same_bits(res[True], res[False], "pinball x 5")


def test_bf16_equals_the_split_path_bit_for_bit():
    res = {}
    for fused in (True, False):
        eng, m, cfg, g, (X, coords, t, y) = _engine("default227_learn", fused, grad_clip=0, dtype="bf16")
        for _ in range(3):
            eng.step(X, coords, t, y)
        res[fused] = _state(eng)
        res[fused]["bf16"] = eng._shadow_buf.clone()       # the operand copies the MLP group's launch keeps current
        assert torch.isfinite(res[fused]["flat"]).all()
        del eng, m
    _assert_same_bits(res[True], res[False], "bf16")
