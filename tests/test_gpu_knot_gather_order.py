"""Regression test of the per-knot gather of dW0^T (csrc/l1_bwd_body.h) over the switches it already has:

  STDADK_KNOTS_PER_WAVE = 1 | 2   one knot per wave / two neighbouring knots per wave (fixed grid knots)
  STDADK_KNOT_XCD = 0 | 1         table order / XCD-striped order of the knot groups
  STDADK_NO_DW_ALL                the stand-alone l1_window_backward launch instead of the merged weight-gradient launch

A knot sums its own rows in sorted order whichever wave, workgroup or launch owns it, and fmaf(0, dz, acc) == acc for the
padding and for the partner knot's rows, so

  a. every gradient of stdadk_train_fwd_bwd_f32 -- the rows of dW0^T among them, and on the learnable path the knot
     gradients stdadk_knot_backward_f32 forms from kpart -- is bit-identical over the four combinations of the first two
     switches, flipped between calls in one process, and over the two launches; rows of knots that no row of the batch
     reaches are exactly 0;
  b. on the learnable path the knot gradients (d_cx, d_cy, d_log_bw: the gather's kpart sums finished per knot) agree
     with float64 per knot in both orders and both launches, with the comparator and the recorded bound of
     golden/knot_cases.py as they stand (compare_knots, bounds() from knot_achieved.json) on its own window cases.

What the merged launch of this tree changes against its parent is its occupancy (four workgroups per CU): the merged
launch against the stand-alone one is the comparison that touches it.  Not covered here: the parameters after a
one-call step and STDADK_DW_FIN=2 over scheduling switches -- the switches those cases were for (coarse knot groups in
front of the GEMM tiles, two row groups in flight, profiles/knot_gather_chains.md) are not in the tree, and the
existing switches change the number of knot workgroups, hence the squared-norm slots and the rounding of the clip
coefficient.

Shapes of a: grid sides [5, 9, 11] (odd, no multiple of 8, unequal XCD lists, absent pair partners), [8, 16, 24],
[32, 64, 72]; rows 1 .. 1 024 around the list's group sizes; H = 128 and 256; rows uniform, all at one point (one knot
pair gets every row: more than BW_LIST entries, mid-walk flushes, every remainder class of the final flush), half the
domain empty, on the border and on knots.  Each test prints what it compared (-s).
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

from golden import cases
from golden import knot_cases as kc
from oracle import stdadk_oracle as orc

import test_gpu_knot_gradients as KG
import test_gpu_parity as T

pytestmark = pytest.mark.gpu

GRIDS = {"odd": [5, 9, 11], "mid": [8, 16, 24], "c2": [32, 64, 72]}
ROWS = [1, 8, 9, 16, 17, 64, 65, 257, 1024]
POINT_ROWS = ROWS + [72, 79, 1023]          # at one point: 8 and 15 modulo 16 above BW_LIST, 15 modulo 16 after many flushes
LAYOUTS = ["uniform", "point", "half", "border"]
COMBOS = [(nk, x) for nk in ("2", "1") for x in ("1", "0")]          # (STDADK_KNOTS_PER_WAVE, STDADK_KNOT_XCD)
K_TEMPORAL = [10, 15]
SWITCHES = ("STDADK_KNOTS_PER_WAVE", "STDADK_KNOT_XCD", "STDADK_NO_DW_ALL")


@contextlib.contextmanager
def _env(**kw):
    """The library reads these per launch (getenv): set for one call, restored behind it."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in kw.items():
            assert k in SWITCHES
            os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _cfg(grid, H, B=0, basis="wendland", learnable=False):
    return dict(p=0, k_spatial_centers=[s * s for s in GRIDS[grid]], k_temporal_centers=K_TEMPORAL, hidden_dims=[H, 64],
                layernorm=True, basis=basis, output_dim=1, B=B, seed=600 + 7 * len(grid) + H, learnable=learnable)


@functools.lru_cache(maxsize=None)
def _state(grid, H, basis="wendland"):
    return cases.make_state(_cfg(grid, H, basis=basis))


def _model(grid, H, basis="wendland", learnable=False):
    from stnf.models import STInterpMLP
    cfg = _cfg(grid, H, basis=basis, learnable=learnable)
    m = STInterpMLP(p=0, k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=K_TEMPORAL,
                    hidden_dims=cfg["hidden_dims"], dropout=0.0, layernorm=True, spatial_learnable=learnable,
                    spatial_basis_function=basis, output_dim=1)
    sd = m.state_dict()
    for k, v in _state(grid, H, basis).items():
        sd[k] = torch.from_numpy(v.copy())
    m.load_state_dict(sd)
    if learnable:
        dc, dlb = cases.knot_perturbation(cfg)
        with torch.no_grad():
            m.spatial_basis.centers.add_(torch.from_numpy(dc))
            m.spatial_basis.log_bandwidths.add_(torch.from_numpy(dlb))
    m.force_window_path = True
    return m.to(T.dev())


_MODELS = {}


def _shared_model(grid, H, basis="wendland", learnable=False):
    key = (grid, H, basis, learnable)
    if key not in _MODELS:
        _MODELS[key] = _model(*key)
    return _MODELS[key]


def _batch(layout, B, grid, seed=0):
    """(coords (B, 2), t (B,), y (B, 1)) float32."""
    rs = np.random.RandomState(9000 + 31 * B + seed)
    F = np.float32
    coords = rs.uniform(0.0, 1.0, (B, 2)).astype(F)
    if layout == "point":
        coords[:] = F([0.37, 0.61])
    elif layout == "half":
        coords[:, 0] *= F(0.45)
    elif layout == "border":
        centers, _, _ = orc.uniform_knots([s * s for s in GRIDS[grid]])
        edge = np.array([[0, 0], [1, 1], [0, 1], [1, 0], [0, 0.5], [1, 0.25], [0.75, 0], [0.3, 1]], F)
        coords[0::2] = edge[np.arange(len(coords[0::2])) % len(edge)]
        pick = rs.randint(0, len(centers), size=len(coords[1::2]))
        coords[1::2] = centers[pick].astype(F)                     # exactly on knots of every level
    t = rs.uniform(0.0, 1.0, B).astype(F)
    y = rs.standard_normal((B, 1)).astype(F)
    return coords, t, y


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(T.dev())


def _grads(m, coords, t, y, learnable=False):
    """stdadk_train_fwd_bwd_f32 into NaN-prefilled gradients: [dW0^T, ...] (+ d_centers, d_log_bw on the learnable path)."""
    from stnf import _native as N
    d = T.dev()
    B = len(coords)
    st = m._step_state(d)
    assert N.step_uses_window(st.basis, st.desc, st.flags) and st.w0_transposed
    plist = m._body_params()
    grads = [torch.full(tuple(q.shape), float("nan"), device=d) for q in plist]
    grads[0] = torch.full((plist[0].shape[1], plist[0].shape[0]), float("nan"), device=d)
    gt = m._pack(grads)
    ws = torch.empty(N.step_workspace_bytes(st.basis, st.desc, B, st.flags) // 4, device=d, dtype=torch.float32)
    loss_sum = torch.zeros(1, device=d)
    c = _dev(coords)
    N.train_fwd_bwd(st.basis, st.desc, st.params, gt, c, _dev(t), None, _dev(y), B, 1.0 / B, loss_sum, None, ws, st.flags)
    out = list(grads)              # (not the loss: its row blocks add into one float in arrival order, call by call)
    if learnable:
        Ks = m.spatial_basis.k
        dc, dlb = torch.full((Ks, 2), float("nan"), device=d), torch.full((Ks,), float("nan"), device=d)
        N.knot_backward(st.basis, st.desc, st.params, c, B, ws, st.flags, None, dc, dlb, None)
        out += [dc, dlb]
    torch.cuda.synchronize()
    assert all(torch.isfinite(g).all() for g in out) and torch.isfinite(loss_sum).all()
    return out


def _same_over_combos(m, coords, t, y, what, learnable=False, **fixed):
    ref = None
    for nk, xcd in COMBOS:
        with _env(STDADK_KNOTS_PER_WAVE=nk, STDADK_KNOT_XCD=xcd, **fixed):
            got = _grads(m, coords, t, y, learnable)
        if ref is None:
            ref = got
            continue
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (what, f"knots per wave={nk} xcd={xcd}", "tensor", i,
                                       int((a != b).sum().item()), "entries differ")
    return ref


# ------------------------------------------------------------------ a. bit-identity of the gradients
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_gradients_bit_identical_over_bodies_and_orders(grid, layout, H):
    m = _shared_model(grid, H)
    rows = POINT_ROWS if layout == "point" else ROWS
    for B in rows:
        coords, t, y = _batch(layout, B, grid)
        ref = _same_over_combos(m, coords, t, y, (grid, layout, H, B))
        if layout == "half":      # knots beyond the occupied half: exact zero rows, whatever the switches
            centers, bw, _ = orc.uniform_knots([s * s for s in GRIDS[grid]])
            geo = kc.geometry(coords, centers, np.log(bw.astype(np.float64)), "wendland")
            un = np.nonzero(kc.unreached(geo, "wendland"))[0]
            assert un.size > 0
            assert torch.all(ref[0][torch.from_numpy(un).to(T.dev())] == 0.0)
    print(f"{grid} {layout} H={H}: rows {rows}, {len(COMBOS)} combinations, {len(ref)} tensors each, bit-identical")


@pytest.mark.parametrize("grid", list(GRIDS))
def test_stand_alone_launch_bit_identical_to_the_merged_one(grid):
    """l1_window_backward on its own (STDADK_NO_DW_ALL) in every body and order against the merged launch's default."""
    for H in (128, 256):
        m = _shared_model(grid, H)
        for layout, B in (("uniform", 257), ("point", 79), ("point", 1024), ("border", 65), ("half", 17)):
            coords, t, y = _batch(layout, B, grid)
            got = _same_over_combos(m, coords, t, y, (grid, "stand-alone", layout, H, B), STDADK_NO_DW_ALL="1")
            with _env():
                base = _grads(m, coords, t, y)
            for i, (a, b) in enumerate(zip(base, got)):
                assert torch.equal(a, b), (grid, layout, H, B, "differs from the merged launch, tensor", i)
    print(f"{grid}: stand-alone launch bit-identical over the combinations and to the merged launch")


@pytest.mark.parametrize("basis", ["wendland", "triangular"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_learnable_knots_bit_identical_over_orders_and_launches(grid, basis):
    """The KNOTS body: dW0^T, every other gradient and the knot gradients formed from kpart."""
    for H in (128, 256):
        m = _shared_model(grid, H, basis, True)
        for layout, B in (("uniform", 257), ("point", 79), ("point", 1024), ("border", 65)):
            coords, t, y = _batch(layout, B, grid)
            _same_over_combos(m, coords, t, y, (grid, basis, layout, H, B), learnable=True)
            _same_over_combos(m, coords, t, y, (grid, basis, layout, H, B, "stand-alone"), learnable=True,
                              STDADK_NO_DW_ALL="1")
    print(f"{grid} {basis}: learnable-knot gradients bit-identical")


# ------------------------------------------------------------------ b. knot gradients per knot against float64
ROUTES = {"merged_striped": {}, "merged_table_order": dict(STDADK_KNOT_XCD="0"),
          "stand_alone_striped": dict(STDADK_NO_DW_ALL="1"),
          "stand_alone_table_order": dict(STDADK_NO_DW_ALL="1", STDADK_KNOT_XCD="0")}


@pytest.mark.parametrize("case", kc.WINDOW_CASES, ids=lambda c: c["name"])
def test_knot_gradients_per_knot_against_float64_in_every_order_and_launch(case):
    """knot_cases' window cases (a knot one row reaches, ragged row counts, more rows than BW_LIST, unreached knots)
    through kc.compare_knots with kc.bounds(), unchanged, once per order and launch; bit-identical between them."""
    inp = kc.step_inputs(case)
    ev = kc.step_eval(kc.step_data(case, inp), None)
    m = KG._build(case, inp)
    B = len(inp["coords"])
    first = None
    for route, env in ROUTES.items():
        with _env(**env):
            st, ws, coords, _, keep = KG._backward(m, case, inp)
            dc, dlb = KG._knot_backward(m, st, ws, coords, B, None)
            torch.cuda.synchronize()
        w = kc.compare_knots(dc.cpu().numpy(), dlb.cpu().numpy(), ev)
        print(f"{case['name']} [{route}]: {kc.fmt(w)}")
        if first is None:
            first = (dc, dlb)
        else:
            assert torch.equal(first[0], dc) and torch.equal(first[1], dlb), (case["name"], route)
