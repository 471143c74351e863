"""The layer-0 window path on SITE-STRUCTURED batches against float64 (tests/golden/site_cases.py): rows (site, time)
whose coordinates repeat exactly, clustered, with empty regions, sites on the domain border and exactly on knots.

Every other test that pins the window kernels to the float64 oracle draws uniform coordinates (about one row per
binning cell, every knot reached); the tests with clustered or repeated rows compare one GPU variant with another
that shares every downstream kernel.  What the batches here reach and uniform ones do not:
  * in-cell ordering (bin_small_body, bin_dw_body, cell_order_kernel) with up to 2 000 equal keys in a cell, and the
    16-bit slices of bin_dw_body cutting through one cell;
  * the per-knot gather (l1_window_bwd_body, walk_cell_runs) with thousands of candidates per knot (many BW_LIST
    flushes) and with none: the row of dW0^T must be written as zeros over what the previous step left there;
  * the grouped forward (l1_window_fwd_multi_body) with identical windows and with windows in different clusters;
  * the d > 0 guards of the knot gradients, and knot cells holding dozens of knots that sit on observations.
The comparison (site_cases.compare_step) is the one tests/test_site_cases_cpu.py shows to have teeth.
"""
import time

import numpy as np
import pytest
import torch

from golden import cases
from golden import site_cases as sc
from oracle import stdadk_oracle as orc
from oracle import torch_f64

import test_gpu_parity as T
import test_gpu_large_batch as L

pytestmark = pytest.mark.gpu
TOL = sc.TOL
KNOT_TOL = 2e-5              # gradients on the learnable / scattered paths, as test_learnable_window_follows_moved_knots

_REF = {}


def _dev_batch(b, p):
    d = T.dev()
    X = torch.from_numpy(b["X"]).to(d) if p > 0 else None
    return X, torch.from_numpy(b["coords"]).to(d), torch.from_numpy(b["t"]).to(d), torch.from_numpy(b["y"]).to(d)


def _module_step(m, b, p, loss_fn=None):
    """dict(y, loss, grads) of one module forward + backward."""
    X, coords, t, y = _dev_batch(b, p)
    m.train()
    m.zero_grad()
    if loss_fn is None:
        yp = m(X, coords, t)
        loss = torch.nn.functional.mse_loss(yp, y)
    else:
        yp, loss = loss_fn(X, coords, t, y)
    loss.backward()
    return dict(y=yp.detach().cpu().numpy(), loss=loss.item(),
                grads={k: q.grad.cpu().numpy() for k, q in m.named_parameters()})


# ------------------------------------------------------------------ a. module forward + backward, fixed grid knots
def _module_reference(model, sites):
    if (model, sites) not in _REF:
        cfg, b = sc.module_case(model, sites)
        params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
        yo, lo, go, alts = torch_f64.train_step_grads(b["X"], b["coords"], b["t"], b["y"], params, cfg, device=T.dev(),
                                                      chunk=4096, kink_tol=sc.KINK_TOL)
        _REF[(model, sites)] = (dict(y=yo, loss=lo, grads=go), alts)
    return _REF[(model, sites)]


@pytest.mark.parametrize("group", ["1", "2"])
@pytest.mark.parametrize("model,sites", sc.MODULE_CASES)
def test_module_step_on_site_batches(model, sites, group, monkeypatch):
    """y, loss and every gradient of the window path, one and two observations per wave, against float64; the dW0
    columns of the knots no site reaches exactly zero."""
    from stnf import _native as N
    monkeypatch.setenv("STDADK_L1_GROUP", group)
    cfg, b = sc.module_case(model, sites)
    ref, alts = _module_reference(model, sites)
    m = T.build_model(cfg)
    st = m._step_state(T.dev())
    assert N.step_uses_window(st.basis, st.desc, st.flags)
    got = _module_step(m, b, cfg["p"])
    r = sc.compare_step(got, ref, alts, TOL, sc.max_flipped(model, sites))
    print(f"{model} {sites} group {group}: loss {r['loss']:.1e} y {r['y']:.1e} worst gradient {r['worst']:.2e} "
          f"({r['worst_key']}); {len(alts)} near-kink units, flipped {r['flipped']}; {r['unreached']} unreached columns")
    assert r["unreached"] > 0 or sites == "on_knots"


# ------------------------------------------------------------------ b. one-call steps along a sequence
CARRIERS = ("dw", "adam", "side")


def _sequence_run(name, carrier, monkeypatch, res, dres, record=False):
    """Three one-call steps of a sequence with the next batch announced; each step's loss and gradient against
    float64 at that step's own pre-step parameters.  Returns the final parameters."""
    from stnf import _native as N
    from stnf.engine import TrainStep
    if carrier == "adam":
        monkeypatch.setenv("STDADK_BIN_IN", "adam")
    else:
        monkeypatch.delenv("STDADK_BIN_IN", raising=False)
    B, _ = sc.SEQUENCES[name]
    cfg, o = sc.SEQ_CFG, sc.SEQ_OPT
    d = T.dev()
    batches = sc.sequence_batches(name, res)
    idx = [torch.from_numpy(i).to(d) for i in batches]
    m = T.build_model(cfg).train()
    eng = TrainStep(m, lr=o["lr"], weight_decay=o["weight_decay"], betas=o["betas"], eps=o["eps"],
                    grad_clip=o["grad_clip"], ema_decay=o["ema_decay"], max_batch=B, seed=5,
                    inline_prep=carrier != "side")
    assert eng._whole_step and eng.uses_window
    reached1 = None
    for i, ib in enumerate(idx):
        nxt = idx[i + 1] if i + 1 < len(idx) else None
        torch.cuda.synchronize()
        key = (name, i)
        if key not in _REF or not torch.equal(_REF[key][0], eng.flat):
            b = sc.take(res, batches[i])
            params = L._views(eng, m, eng.flat)
            yo, lo, go, alts = torch_f64.train_step_grads(None, b["coords"], b["t"], b["y"], params, cfg, device=d,
                                                          chunk=4096, kink_tol=sc.KINK_TOL)
            _REF[key] = (eng.flat.clone(), dict(y=yo, loss=lo, grads=go), alts)
        _, ref, alts = _REF[key]
        if record and i == 1:
            N.profile_enable(True)
        t0 = time.perf_counter()
        eng.step_indexed(dres[0], dres[1], dres[2], ib, next_idx=nxt)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if record and i == 1:
            names = [k for k, _ in N.profile_collect()]
            N.profile_enable(False)
            print(f"{name} {carrier} step 2 launches: {names}")
        if nxt is not None:
            assert eng._prepared is not None
            assert eng._prepared.inline == (nxt.numel() <= 4096 and carrier != "side"), (carrier, i)
        assert int(eng.step_dev.item()) == i + 1
        got = dict(y=None, loss=eng.mean_loss(), grads=L._views(eng, m, eng.grad))
        norm = float(np.sqrt(sum(float((g * g).sum()) for g in ref["grads"].values())))
        assert norm > 1.5 * o["grad_clip"]                       # clipping active
        r = sc.compare_step(got, ref, alts, TOL, sc.SEQ_MAX_FLIPPED[name][i])
        now = sc.reached(ref["grads"]["mlp.0.weight"])
        print(f"{name} {carrier} step {i + 1}: B {B} rows/cell {sc.rows_per_cell(sc.take(res, batches[i])['coords'])} "
              f"wall {wall * 1e3:.2f} ms; loss {r['loss']:.1e} worst gradient {r['worst']:.2e} ({r['worst_key']}); "
              f"{len(alts)} near-kink units, flipped {r['flipped']}; {r['unreached']} unreached columns")
        if i == 0:
            reached1 = now
        else:
            # the stale-row check: step 1 has just written non-zero rows of dW0^T for these knots
            stale = reached1 & ~now
            assert stale.sum() > 1000 and not (now & ~reached1).any()
            assert np.all(got["grads"]["mlp.0.weight"][:, stale] == 0.0)
    torch.cuda.synchronize()
    return eng.flat.clone()


@pytest.fixture(scope="module")
def resident():
    res = sc.resident()
    d = T.dev()
    return res, tuple(torch.from_numpy(res[k]).to(d) for k in ("coords", "t", "y"))


def test_sequence_4096_three_carriers(resident, monkeypatch):
    """4 096 rows, the most bin_dw_body holds: the next batch (a crowded cell of ~1 900 rows) binned by the
    weight-gradient launch, by the optimiser launch and on the side stream; the three end in equal parameters."""
    res, dres = resident
    flats = {c: _sequence_run("seq4096", c, monkeypatch, res, dres, record=c == "dw") for c in CARRIERS}
    for c in ("dw", "adam"):
        assert torch.equal(flats[c], flats["side"]), c


@pytest.mark.parametrize("name", ["seq4097", "seq8192", "seq8193"])
def test_sequence_larger_batches(name, resident, monkeypatch):
    """4 097: declined by the step, prepared on the side stream; 8 192: the bin_small limit; 8 193: multi-kernel
    binning on a 128 x 128 grid."""
    res, dres = resident
    _sequence_run(name, "dw", monkeypatch, res, dres)


def test_one_cell_step_time_is_printed(resident):
    """Wall time of a 4 096-row step with ~1 900 rows in one cell next to a uniform 4 096-row step (no pass/fail on
    the time: the in-cell order costs n^2 per cell on one thread; profiles/site_batches.md records the figures)."""
    from stnf.engine import TrainStep
    res, dres = resident
    d = T.dev()
    cfg, o = sc.SEQ_CFG, sc.SEQ_OPT
    crowded = torch.from_numpy(sc.sequence_batches("seq4096", res)[1]).to(d)
    ucfg = dict(cfg, B=4096, seed=99)
    _, uc, ut, uy = cases.make_inputs(ucfg)
    uni = tuple(torch.from_numpy(a).to(d) for a in (uc, ut.reshape(-1), uy))
    uidx = torch.arange(4096, device=d)
    out = {}
    for label, data, ib in (("one_cell", dres, crowded), ("uniform", uni, uidx)):
        eng = TrainStep(T.build_model(cfg).train(), lr=o["lr"], grad_clip=o["grad_clip"], ema_decay=o["ema_decay"],
                        max_batch=4096, seed=5)
        times = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.step_indexed(data[0], data[1], data[2], ib, next_idx=ib)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        out[label] = min(times[1:])
        assert np.isfinite(eng.mean_loss())
    print(f"4096-row one-call step, wall: one_cell {out['one_cell'] * 1e3:.3f} ms, uniform {out['uniform'] * 1e3:.3f} ms")


# ------------------------------------------------------------------ c. learnable grid knots
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("sites", ["on_knots", "one_cell"])
@pytest.mark.parametrize("name", ["default227_learn", "c2_b257_learn"])
def test_learnable_knots_on_site_batches(name, sites, dense):
    """Perturbed learnable grid knots (cases.knot_perturbation) with observations exactly ON the perturbed float32
    centres (d == 0: the guards of the knot-gradient gather) and crowded into one cell: y, the loss with its
    penalties and every gradient -- centres and log-bandwidths included, all finite -- against the oracle, on the
    window and on the materialising path."""
    m, cfg, kn, g = T.build_learn_model(name)
    m.force_dense_path = dense
    m.force_window_path = not dense
    cen = m.spatial_basis.centers.detach().cpu().numpy()
    B = 1003
    b = sc.batch(sc.site_set(sites, cfg, cen), B, 8100 + len(name) + len(sites), cfg["p"])
    if sites == "on_knots":                                      # every row at distance exactly 0 from a knot
        assert ((np.abs(b["coords"][:, None, :] - cen[None, :, :]).sum(-1) == 0).sum(1) >= 1).all()

    def loss_fn(X, coords, t, y):
        yp = m(X, coords, t)
        loss = torch.nn.functional.mse_loss(yp, y)
        if kn.get("domain_penalty_weight", 0.0) > 0:
            loss = loss + kn["domain_penalty_weight"] * m.compute_domain_penalty()
        if kn.get("movement_penalty_weight", 0.0) > 0:
            loss = loss + kn["movement_penalty_weight"] * m.compute_movement_penalty()
        return yp, loss

    got = _module_step(m, b, cfg["p"], loss_fn)
    for k, v in got["grads"].items():
        assert np.isfinite(v).all(), k
    params = dict(cases.make_state(cfg))
    params["spatial_basis.centers"] = cen
    params["spatial_basis.log_bandwidths"] = m.spatial_basis.log_bandwidths.detach().cpu().numpy()
    yo, lo, go = orc.learnable_step_grads(b["X"], b["coords"], b["t"], b["y"], params, dict(cfg, B=B), kn,
                                          g["in_centers_init"])
    r = sc.compare_step(got, dict(y=yo, loss=lo, grads=go), [], TOL, 0, grad_tol=KNOT_TOL)
    print(f"{name} {sites} {'dense' if dense else 'window'}: loss {r['loss']:.1e} y {r['y']:.1e} worst gradient "
          f"{r['worst']:.2e} ({r['worst_key']}); {r['unreached']} unreached columns")


# ------------------------------------------------------------------ d. scattered knots taken from the sites
def _site_knot_model(learnable, seed=91):
    from stnf.models import STInterpMLP
    pts = sc.blobs(6000, 305)
    np.random.seed(seed)
    cfg = dict(p=0, k_spatial_centers=[1024, 4096], k_temporal_centers=[10, 15], hidden_dims=[256, 128],
               layernorm=True, basis="wendland", output_dim=1, B=1003, seed=seed)
    m = STInterpMLP(p=0, k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=cfg["k_temporal_centers"],
                    hidden_dims=cfg["hidden_dims"], dropout=0.0, layernorm=True, spatial_learnable=learnable,
                    spatial_init_method="random_site", spatial_basis_function="wendland", train_coords=pts)
    st = cases.make_state(cfg)
    with torch.no_grad():
        for k, q in m.named_parameters():
            if k in st:
                q.copy_(torch.from_numpy(st[k].copy()))
    m.force_window_path = True
    return m.to(T.dev()), cfg, st, pts


@pytest.mark.parametrize("learnable", [True, False])
def test_scattered_knots_from_sites(learnable):
    """random_site knots (1 024 + 4 096) drawn from 6 000 clustered sites, batches from the same sites: knots sit
    exactly on observations and one knot cell holds dozens of knots.  Window path against the oracle, bounds as
    test_scattered_knots_window_path_matches_materialised_and_oracle."""
    from stnf import _native as N
    m, cfg, st, pts = _site_knot_model(learnable)
    d = T.dev()
    desc = m._basis_desc()
    assert desc.n_levels == 2 and desc.side[0] == 1024 and desc.side[1] == 4096
    st_ = m._step_state(d)
    assert N.step_uses_window(st_.basis, st_.desc, st_.flags)
    sb = m.spatial_basis
    cen = sb.centers.detach().cpu().numpy()
    b = sc.batch(pts, cfg["B"], 8200)
    assert (np.abs(b["coords"][:, None, :] - cen[None, :1024, :]).sum(-1) == 0).any()
    kc = orc.cell_keys(cen[1024:], 32)
    assert np.bincount(kc).max() >= 24
    got = _module_step(m, b, 0)
    for k, v in got["grads"].items():
        assert np.isfinite(v).all(), k
    if learnable:
        params = dict(st)
        params["spatial_basis.centers"] = cen
        params["spatial_basis.log_bandwidths"] = sb.log_bandwidths.detach().cpu().numpy()
        yo, lo, go = orc.learnable_step_grads(b["X"], b["coords"], b["t"], b["y"], params, cfg, {}, cen)
    else:
        tc, tb = m.temporal_basis.centers.cpu().numpy(), m.temporal_basis.bandwidths.cpu().numpy()
        feat = orc.features(b["X"], orc.spatial_basis(b["coords"], cen.astype(np.float64), sb.bandwidths.cpu().numpy(),
                                                      "wendland"), orc.temporal_basis(b["t"], tc, tb), 0)
        yo, cache = orc.mlp_forward(feat, st, len(cfg["hidden_dims"]), True)
        go = orc.mlp_mse_backward(yo, b["y"], cache, st, len(cfg["hidden_dims"]), True)
        lo = orc.mse(yo, b["y"])
    r = sc.compare_step(got, dict(y=yo, loss=lo, grads=go), [], TOL, 0, grad_tol=KNOT_TOL)
    print(f"scattered from sites, learnable {learnable}: loss {r['loss']:.1e} y {r['y']:.1e} worst gradient "
          f"{r['worst']:.2e} ({r['worst_key']}); {r['unreached']} unreached columns")


# ------------------------------------------------------------------ e. binning integers
@pytest.mark.parametrize("B,G", sc.BIN_CASES)
def test_bin_obs_on_site_batches(B, G):
    """Cell keys, cell starts and the permutation (ascending batch position inside a cell) of batches with a cell of
    ~1 900 equal-keyed rows, clustered and border sites: bit-exact against the oracle and a stable argsort."""
    from stnf import _native as N
    coords = sc.bin_batch(B)["coords"]
    assert 1000 <= sc.rows_per_cell(coords, G) <= sc.MAX_ROWS_PER_CELL
    keys, cell_start, perm = N.bin_obs(torch.from_numpy(coords).to(T.dev()), G)
    ko = orc.cell_keys(coords, G)
    assert np.array_equal(keys.cpu().numpy(), ko)
    counts = np.bincount(ko, minlength=G * G)
    assert np.array_equal(cell_start.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    assert np.array_equal(perm.cpu().numpy(), np.argsort(ko, kind="stable").astype(np.int32))


# ------------------------------------------------------------------ f. grid prediction
@pytest.mark.parametrize("sites", ["on_knots", "border", "one_cell"])
def test_predict_grid_on_sites_against_float64(sites):
    """Predictor.predict_grid (per-site half of layer 0 + per-time half) on sites x 7 times against the float64
    forward of the expanded rows."""
    from stnf.engine import Predictor
    cfg = cases.MODEL_CASES["c2_b257"]
    d = T.dev()
    m = T.build_model(cfg)
    m.eval()
    s = sc.site_set(sites, cfg)
    S, Tn = len(s), 7
    tv = (np.arange(Tn, dtype=np.float32) / np.float32(Tn - 1)).astype(np.float32)
    got = Predictor(m, chunk=32768).predict_grid(torch.from_numpy(s).to(d), torch.from_numpy(tv).to(d))
    assert got.shape == (Tn, S, 1)
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    yo = orc.model_forward(None, np.tile(s, (Tn, 1)), np.repeat(tv, S).reshape(-1, 1), params, cfg)[0]
    err = np.abs(got.cpu().numpy().reshape(-1, 1) - yo).max()
    print(f"predict_grid {sites}: S {S} max |y - y64| {err:.2e}")
    assert err <= TOL * max(1.0, np.abs(yo).max())
