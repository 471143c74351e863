"""The gradients into the learnable knots (centres, log-bandwidths) PER KNOT against float64 (tests/golden/knot_cases.py):

    |got - ref| <= K 2^-24 S[knot, output]

with S the sum of the magnitudes of what is added to form the output and K four times what a float32 restatement of
the formulas achieves (golden/knot_achieved.json); outputs whose scale is 0 -- every data gradient of a compact-support
knot that no row reaches -- exactly 0.0; everything finite.  Every other test of these gradients asserts one rel-L2
per tensor, which a fault in one knot, one row or one branch of the finish passes (tests/test_knot_cases_cpu.py shows
nine such faults this comparator rejects).

  a. stdadk_knot_grad_f32 on its own: the ragged last 64-knot tile, one slab .. the 32-slab cap and rows per slab
     beyond 128, B not a multiple of the four waves, B in {0, 1}, ld > Ks with an unaligned base.
  b. stdadk_knot_backward_f32 after a real stdadk_train_fwd_bwd_f32, materialising and window route each against
     float64, with and without a stdadk_knot_train in every setting of knot_cases.KT_SETTINGS; the penalty's share of
     the loss; scattered learnable knots on the window route.
  c. the module's autograd (SpatialBasisEmbedding, learnable) above the slab cap.

Everything goes through stnf._native; outputs are prefilled with NaN before each call (the ABI says "overwritten").
Each test prints the worst normalised error per output and the knot it occurred at (-s).
"""
import numpy as np
import pytest
import torch

from golden import cases
from golden import knot_cases as kc

import test_gpu_parity as T
import test_gpu_round2 as R2

pytestmark = pytest.mark.gpu
LOSS_TOL = 1e-5              # BASELINE.json's bound, as everywhere


def _nan(*shape):
    return torch.full(shape, float("nan"), device=T.dev(), dtype=torch.float32)


def _to(a):
    if a.size == 0:          # (torch.from_numpy gives an empty array strides of its own)
        return torch.empty(a.shape, device=T.dev(), dtype=torch.float32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(T.dev())


# ------------------------------------------------------------------ a. stdadk_knot_grad_f32 on its own
@pytest.mark.parametrize("case", kc.EMB_CASES, ids=lambda c: c["name"])
def test_knot_grad_per_knot(case):
    from stnf import _native as N
    B, Ks = case["B"], case["Ks"]
    inp = kc.emb_inputs(case)
    ev = kc.emb_eval(case, inp)
    coords, centers, log_bw = _to(inp["coords"]), _to(inp["centers"]), _to(inp["log_bw"])
    pad, first = kc.EMB_WIDE
    wide = _nan(B, Ks + pad)
    view = wide[:, first:first + Ks]
    view.copy_(_to(inp["G"]))
    assert B == 0 or (view.stride(0) == Ks + pad > Ks and view.data_ptr() % 16 != 0)
    first_bits = None
    for label, d_phi in (("contiguous", _to(inp["G"])), ("ld > Ks", view)):
        dc, dlb = _nan(Ks, 2), _nan(Ks)
        N.knot_grad(coords, d_phi, centers, log_bw, case["basis"], dc, dlb)
        dc, dlb = dc.cpu().numpy(), dlb.cpu().numpy()
        if first_bits is None:
            first_bits = (dc.copy(), dlb.copy())
        else:        # the row stride changes addresses, not arithmetic
            assert np.array_equal(dc, first_bits[0], equal_nan=True) and np.array_equal(dlb, first_bits[1], equal_nan=True)
        if B == 0:
            assert np.all(dc == 0.0) and np.all(dlb == 0.0)
        w = kc.compare_knots(dc, dlb, ev)
        print(f"{case['name']} [{label}]: {kc.fmt(w)}; {int(ev['unreached'].sum())} unreached knots")


# ------------------------------------------------------------------ b. stdadk_knot_backward_f32 after a real backward
def _build(case, inp):
    from stnf.models import STInterpMLP
    cfg = inp["cfg"]
    m = STInterpMLP(p=cfg["p"], k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=cfg["k_temporal_centers"],
                    hidden_dims=cfg["hidden_dims"], dropout=0.0, layernorm=cfg["layernorm"], spatial_learnable=True,
                    spatial_basis_function=cfg["basis"], output_dim=cfg["output_dim"])
    sb = m.spatial_basis
    assert np.array_equal(sb.centers_init.numpy(), inp["centers_init"])
    names = [k for k, _ in m.named_parameters()]
    assert names[:2] == ["spatial_basis.centers", "spatial_basis.log_bandwidths"] and names[2:] == list(inp["state"])
    with torch.no_grad():
        sb.centers.copy_(torch.from_numpy(inp["centers"]))
        sb.log_bandwidths.copy_(torch.from_numpy(inp["log_bw"]))
        for k, q in list(m.named_parameters())[2:]:
            q.copy_(torch.from_numpy(inp["state"][k].copy()))
    m.force_dense_path = case["route"] == "dense"
    m.force_window_path = case["route"] == "window"
    return m.to(T.dev())


def _backward(m, case, inp):
    """stdadk_train_fwd_bwd_f32 on the model's step state: (state, workspace, coords, loss_sum after the data term)."""
    from stnf import _native as N
    d = T.dev()
    cfg, B = inp["cfg"], len(inp["coords"])
    st = m._step_state(d, force_dense=m.force_dense_path)
    assert N.step_uses_window(st.basis, st.desc, st.flags) == (case["route"] == "window")
    plist = m._body_params()
    grads = [_nan(*q.shape) for q in plist]
    if st.w0_transposed:
        grads[0] = _nan(plist[0].shape[1], plist[0].shape[0])
    gt = m._pack(grads)
    ws = torch.empty(N.step_workspace_bytes(st.basis, st.desc, B, st.flags) // 4, device=d, dtype=torch.float32)
    coords, t, y = _to(inp["coords"]), _to(inp["t"]).view(-1), _to(inp["y"])
    X = _to(inp["X"]) if cfg["p"] > 0 else None
    loss_sum = torch.zeros(1, device=d)
    Q = cfg["output_dim"]
    N.train_fwd_bwd(st.basis, st.desc, st.params, gt, coords, t, X, y, B, 1.0 / (B * Q), loss_sum, None, ws, st.flags)
    torch.cuda.synchronize()
    assert all(torch.isfinite(g).all() for g in grads)
    return st, ws, coords, loss_sum, (grads, gt)


def _knot_backward(m, st, ws, coords, B, kt_name, loss_sum=None):
    from stnf import _native as N
    Ks = m.spatial_basis.k
    kt = None
    if kt_name is not None:
        s = kc.KT_SETTINGS[kt_name]
        kt = N.make_knot_train(m.spatial_basis.centers_init, s["damping"], s["thr"], s["strength"], s["dom_w"], s["mov_w"],
                               penalty_grad_scale=s["pgs"], penalty_loss_scale=float(B * m.output_dim))
    dc, dlb = _nan(Ks, 2), _nan(Ks)
    N.knot_backward(st.basis, st.desc, st.params, coords, B, ws, st.flags, kt, dc, dlb, loss_sum)
    return dc, dlb


def _check_step_case(case, inp, m, repeat=False):
    """One backward, then the knot gradients without a knot_train and under every KT_SETTINGS entry."""
    d = T.dev()
    B = len(inp["coords"])
    data = kc.step_data(case, inp)
    st, ws, coords, loss_sum, keep = _backward(m, case, inp)
    data_term = float(loss_sum.item())
    assert abs(data_term / (B * m.output_dim) - data["loss"]) <= LOSS_TOL * data["loss"], (data_term, data["loss"])
    worst = {k: (0.0, -1, "") for k in kc.OUTPUTS}
    for kt_name in [None] + list(kc.KT_SETTINGS):
        ev = kc.step_eval(data, kt_name)
        s = kc.KT_SETTINGS[kt_name] if kt_name else None
        acc = torch.zeros(1, device=d) if (s and s["loss"]) else None
        dc, dlb = _knot_backward(m, st, ws, coords, B, kt_name, acc)
        w = kc.compare_knots(dc.cpu().numpy(), dlb.cpu().numpy(), ev)
        for k in kc.OUTPUTS:
            if w[k][0] > worst[k][0]:
                worst[k] = (w[k][0], w[k][1], str(kt_name))
        if acc is not None:
            # the penalty's share of the objective, into an accumulator of its own: penalty_loss_scale x the weighted
            # penalties of float64; with both weights 0 nothing is added at all
            want = B * m.output_dim * ev["penalty"]
            got = float(acc.item())
            if s["dom_w"] == 0.0 and s["mov_w"] == 0.0:
                assert got == 0.0
                same = loss_sum.clone()
                _knot_backward(m, st, ws, coords, B, kt_name, same)
                assert torch.equal(same, loss_sum)                       # exactly unchanged on top of the data term
            else:
                assert want > 0 and abs(got - want) <= LOSS_TOL * want, (case["name"], kt_name, got, want)
                total = loss_sum.clone()
                _knot_backward(m, st, ws, coords, B, kt_name, total)
                assert abs(float(total.item()) - (data_term + want)) <= LOSS_TOL * (data_term + want)
    if repeat:
        a = _knot_backward(m, st, ws, coords, B, "thr02_s1_half")
        b = _knot_backward(m, st, ws, coords, B, "thr02_s1_half")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    print(f"{case['name']}: " + ", ".join(f"{k} {worst[k][0]:.2f} (knot {worst[k][1]}, knot_train {worst[k][2]})"
                                          for k in kc.OUTPUTS)
          + f"; {int(data['unreached'].sum())} unreached knots; rows per knot up to {int(data['geo']['reach'].sum(0).max())}")
    return worst


@pytest.mark.parametrize("case", kc.DENSE_CASES, ids=lambda c: c["name"])
def test_knot_backward_dense_route_per_knot(case):
    inp = kc.step_inputs(case)
    _check_step_case(case, inp, _build(case, inp), repeat=case["name"] == "dense_wendland_h32_p3_B257")


@pytest.mark.parametrize("case", kc.WINDOW_CASES, ids=lambda c: c["name"])
def test_knot_backward_window_route_per_knot(case):
    inp = kc.step_inputs(case)
    _check_step_case(case, inp, _build(case, inp), repeat=case["name"] == "window_wendland_h256_p3_B1003")


def test_knot_backward_scattered_knots_window_route():
    """Scattered learnable knots (1 024 + 4 096 drawn from sites, three pushed out of the unit square, two with inflated
    bandwidths) on the window route, 300 rows: the knot cell lists instead of the grid indexing."""
    from stnf import _native as N
    B = 300
    m, cfg, state = R2._scattered_model([1024, 4096], "wendland", True, 77)
    cfg = dict(cfg, B=B, learnable=True)
    X, coords, t, y = cases.make_inputs(cfg)
    sb = m.spatial_basis
    centers, log_bw = sb.centers.detach().cpu().numpy(), sb.log_bandwidths.detach().cpu().numpy()
    coords = coords.copy()
    kc.redraw(np.random.RandomState(771), coords, centers, log_bw, "wendland", 6,
              lambda geo: kc.near_edge(geo, "wendland").any(1))
    params = dict(state)
    params["spatial_basis.centers"], params["spatial_basis.log_bandwidths"] = centers, log_bw
    inp = dict(cfg=cfg, X=X, coords=coords, t=t, y=y, state=state, centers=centers,
               centers_init=sb.centers_init.cpu().numpy(), log_bw=log_bw, params=params)
    case = dict(name="scattered_wendland_h256_p0_B300", level="step", route="window", basis="wendland", B=B, p=0)
    data = kc.step_data(case, inp)
    assert not kc.near_edge(data["geo"], "wendland").any() and data["unreached"].sum() >= kc.MIN_UNREACHED
    m.force_dense_path, m.force_window_path = False, True
    desc = m._basis_desc()
    assert desc.n_levels == 2 and desc.side[0] == 1024 and desc.side[1] == 4096
    assert m._step_state(T.dev()).flags & N.FLAG_SCATTERED
    _check_step_case(case, inp, m)


# ------------------------------------------------------------------ c. the module's own autograd
@pytest.mark.parametrize("case", kc.MODULE_CASES, ids=lambda c: c["name"])
def test_module_autograd_per_knot_above_the_slab_cap(case):
    """SpatialBasisEmbedding(learnable) -> (phi * w).sum().backward() at 4 225 rows: 32 slabs of 133 rows."""
    from stnf.models.st_interp import SpatialBasisEmbedding
    inp = kc.emb_inputs(case)
    ev = kc.emb_eval(case, inp)
    sb = SpatialBasisEmbedding(n_centers=list(case["grid"]), learnable=True, basis_function=case["basis"]).to(T.dev())
    assert sb.k == case["Ks"]
    with torch.no_grad():
        sb.centers.copy_(_to(inp["centers"]))
        sb.log_bandwidths.copy_(_to(inp["log_bw"]))
    phi = sb(_to(inp["coords"]))
    assert phi.requires_grad and phi.shape == (case["B"], case["Ks"])
    (phi * _to(inp["G"])).sum().backward()
    w = kc.compare_knots(sb.centers.grad.cpu().numpy(), sb.log_bandwidths.grad.cpu().numpy(), ev)
    print(f"{case['name']}: {kc.fmt(w)}; {int(ev['unreached'].sum())} unreached knots")
