"""Basis diagnostics on the device: stdadk_basis_diag_f32 through the ABI on every generated case of
tests/golden/basis_diag_cases.py against the long-double restatement -- N, COVER and both NEAR2 EXACT, every sum within
2^-52 (n want + 64 A), every slot of both outputs compared on pre-filled accumulators -- the boundary cases,
determinism, empty sides and every error code; stdadk_group_norms_f32 in both layouts; the tie to the model's own
float32 basis; then end to end: Predictor.basis_diagnostics on a trained learnable model against the host route on the
tables read back, and grid_scores' `basis` entry."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from golden import basis_diag_cases as bc
import test_gpu_parity as T

pytestmark = pytest.mark.gpu


def run(case, fill=-7.0):
    """One call on pre-filled accumulators (both are ASSIGNED); returns the device tensors (knot_acc, site_acc)."""
    from stnf import _native as N
    d = T.dev()
    Ks, S, L = case["centers"].shape[0], case["coords"].shape[0], len(case["sizes"])
    knot = torch.full((Ks, 7), fill, dtype=torch.float64, device=d)
    site = torch.full((S, L, 3), fill, dtype=torch.float64, device=d)
    ws = torch.empty(N.basis_diag_workspace_bytes(S, Ks) // 8, dtype=torch.float64, device=d)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(d)      # noqa: E731
    N.basis_diag(to(case["centers"]), to(case["bw"]), case["basis"], case["sizes"], to(case["coords"]), to(case["w"]),
                 to(case["v"]), case["rho"], knot, site, ws)
    return knot, site


@pytest.mark.parametrize("basis", bc.BASES)
def test_kernel_matches_the_restatement_on_every_case(basis):
    cases = bc.all_cases(basis)
    outs = [run(c) for c in cases]                               # (the launches are all queued before the reads)
    worst, pairs = 0.0, 0
    for case, (knot, site) in zip(cases, outs):
        rk, rsite, aux = bc.restate_longdouble(case)
        got_k, got_s = knot.cpu().numpy(), site.cpu().numpy()
        bad, ratio = bc.compare(got_k, got_s, rk, rsite, aux)
        print(f"{basis} S={case['coords'].shape[0]} Ks={case['centers'].shape[0]} levels={case['sizes']}: "
              f"worst |delta| / bound = {ratio:.4f}")
        assert not bad, (case["coords"].shape, case["centers"].shape, case["sizes"], bad[:5])
        if case["v"] is None:
            assert not got_k[:, [bc.K_SV, bc.K_WV]].any()
        worst = max(worst, ratio)
        pairs += int(np.asarray(rsite[:, :, bc.S_COVER], dtype=np.float64).sum())
    assert pairs > 0
    print(f"{basis}: {len(cases)} cases, {pairs} pairs in support, worst |delta| / bound = {worst:.4f}")


def test_boundary_cases_on_the_device():
    for case, want in (bc.dyadic_boundary_case(), bc.searched_boundary_case("triangular"),
                       bc.searched_boundary_case("gaussian")):
        knot, site = (a.cpu().numpy() for a in run(case))
        assert np.array_equal(site[:, 0, bc.S_COVER], want.astype(np.float64)), case["basis"]
        assert knot[0, bc.K_N] == want.sum() and knot[0, bc.K_W] == want.sum()
        rk, rsite, aux = bc.restate_longdouble(case)
        assert not bc.compare(knot, site, rk, rsite, aux)[0]


def test_same_call_same_bits():
    case = bc.make_case(1090, 600, (3, 70, 527), "gaussian", seed=77, toggle=3)
    a = [x.cpu().numpy() for x in run(case, fill=-7.0)]
    b = [x.cpu().numpy() for x in run(case, fill=3.0)]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0][:, bc.K_N].sum() > 0


def test_empty_sides():
    """Ks = 0 writes the sites' neutral rows, S = 0 the knots'; both empty is a call that writes nothing."""
    base = bc.make_case(70, 80, (3, 70, 7), "wendland", seed=5, toggle=3)
    no_knots = dict(base, centers=base["centers"][:0], bw=base["bw"][:0], sizes=(0, 0))
    knot, site = (a.cpu().numpy() for a in run(no_knots))
    assert knot.shape == (0, 7) and np.array_equal(site, np.broadcast_to([0.0, 0.0, np.inf], (70, 2, 3)))
    no_sites = dict(base, coords=base["coords"][:0], w=None, v=None)
    knot, site = (a.cpu().numpy() for a in run(no_sites))
    assert site.shape == (0, 3, 3) and np.array_equal(knot, np.broadcast_to([0.0] * 6 + [np.inf], (80, 7)))
    run(dict(no_knots, coords=base["coords"][:0], w=None, v=None))
    # a level without knots between two with: its rows are neutral, the others' are the two-level answer
    gap = dict(base, sizes=(3, 0, 77), w=None, v=None)
    two = dict(base, sizes=(3, 77), w=None, v=None)
    s3, s2 = run(gap)[1].cpu().numpy(), run(two)[1].cpu().numpy()
    assert np.array_equal(s3[:, [0, 2]], s2) and np.array_equal(s3[:, 1], np.broadcast_to([0.0, 0.0, np.inf], (70, 3)))


def _raw(d, S=20, Ks=30, sizes=(10, 20), basis=0, rho=1.0, n_levels=None, knot_off=0, site_off=0, ws_off=0, ws_short=0,
         w_off=0, alias=None, null=None):
    """The C call itself with one thing wrong; returns (code, whether everything it could have written is untouched)."""
    from stnf import _native as N
    lib = N.lib()
    nK, nS = (Ks if 0 < Ks < 2 ** 20 else 1), (S if 0 < S < 2 ** 20 else 1)      # (a refused size is never indexed)
    centers, bw = torch.zeros(nK, 2, device=d), torch.ones(nK, device=d)
    coords = torch.zeros(nS, 2, device=d)
    w = torch.ones(nS + 1, dtype=torch.float64, device=d)
    L = len(sizes) if n_levels is None else n_levels
    need = lib.stdadk_basis_diag_workspace_bytes(S, Ks)
    knot = torch.full((nK * 7 + 2,), 3.0, dtype=torch.float64, device=d)
    site = torch.full((nS * max(L, 1) * 3 + 2,), 3.0, dtype=torch.float64, device=d)
    ws = torch.full((need // 8 + 2,), 3.0, dtype=torch.float64, device=d)
    ptr = {"centers": centers.data_ptr(), "bw": bw.data_ptr(), "coords": coords.data_ptr(), "w": w.data_ptr() + w_off,
           "knot": knot.data_ptr() + knot_off, "site": site.data_ptr() + site_off, "ws": ws.data_ptr() + ws_off,
           "sizes": (C.c_int64 * max(len(sizes), 1))(*sizes)}
    if alias:
        ptr[alias[0]] = ptr[alias[1]]
    if null:
        ptr[null] = None
    rc = lib.stdadk_basis_diag_f32(ptr["centers"], ptr["bw"], Ks, basis, ptr["sizes"], L, ptr["coords"], S, ptr["w"], None,
                                   rho, ptr["knot"], ptr["site"], ptr["ws"], need - ws_short, None)
    torch.cuda.synchronize()
    return rc, bool((knot == 3.0).all()) and bool((site == 3.0).all()) and bool((ws == 3.0).all())


@pytest.mark.parametrize("what,kw,code", [
    ("S < 0", dict(S=-1), -1), ("Ks = 2^31", dict(Ks=2 ** 31, sizes=(2 ** 31,)), -1), ("unknown basis", dict(basis=3), -1),
    ("n_levels 0", dict(n_levels=0), -1), ("n_levels 9", dict(sizes=(30,) + (0,) * 8), -1),
    ("sizes sum short", dict(sizes=(10, 19)), -1), ("sizes sum long", dict(sizes=(10, 21)), -1),
    ("negative size", dict(sizes=(-5, 35)), -1), ("rho 0", dict(rho=0.0), -1), ("rho < 0", dict(rho=-1.0), -1),
    ("rho inf", dict(rho=float("inf")), -1), ("rho NaN", dict(rho=float("nan")), -1),
    ("NULL knot_acc", dict(null="knot"), -1), ("NULL site_acc", dict(null="site"), -1), ("NULL workspace", dict(null="ws"), -1),
    ("NULL sizes", dict(null="sizes"), -1), ("NULL centers", dict(null="centers"), -1), ("NULL coords", dict(null="coords"), -1),
    ("knot_acc aliases centers", dict(alias=("knot", "centers")), -1), ("site_acc aliases coords", dict(alias=("site", "coords")), -1),
    ("site_acc aliases w", dict(alias=("site", "w")), -1), ("knot_acc aliases the workspace", dict(alias=("knot", "ws")), -1),
    ("site_acc aliases knot_acc", dict(alias=("site", "knot")), -1),
    ("knot_acc misaligned", dict(knot_off=4), -3), ("site_acc misaligned", dict(site_off=4), -3),
    ("w misaligned", dict(w_off=4), -3), ("workspace misaligned", dict(ws_off=4), -3),
    ("workspace short", dict(ws_short=8), -4)])
def test_every_error_code(what, kw, code):
    from stnf import _native as N
    lib = N.lib()
    assert (lib.stdadk_basis_diag_workspace_bytes(-1, 5), lib.stdadk_basis_diag_workspace_bytes(5, 2 ** 31)) == (0, 0)
    assert lib.stdadk_basis_diag_workspace_bytes(0, 0) > 0
    rc, untouched = _raw(T.dev(), **kw)
    assert rc == code and untouched, (what, rc, lib.stdadk_last_error())
    assert _raw(T.dev())[0] == 0                                 # the good call succeeds


@pytest.mark.parametrize("H", [1, 7, 128, 256, 300])
def test_group_norms(H):
    """Both layouts, col0 > 0, an ld larger than the row, out ASSIGNED: within H 2^-52 relative of the float64
    restatement (a sum of H non-negative terms in any order)."""
    from stnf import _native as N
    from stnf.utils import basis_diag as BD
    d = T.dev()
    rs = np.random.RandomState(H)
    D, col0, n = 333, 5, 301
    W = (rs.standard_normal((H, D)) * rs.uniform(0, 2, (1, D))).astype(np.float32)
    W[:, col0 + 3] = 0.0
    want = BD.group_sumsq_host(W, col0, n)
    wide = torch.zeros(H, D + 11, device=d)                      # ld = D + 11
    wide[:, :D] = torch.from_numpy(W).to(d)
    wide_t = torch.zeros(D, H + 5, device=d)                     # ld = H + 5
    wide_t[:, :H] = torch.from_numpy(np.ascontiguousarray(W.T)).to(d)
    for W0, transposed in ((torch.from_numpy(W).to(d), False), (wide[:, :D], False),
                           (torch.from_numpy(np.ascontiguousarray(W.T)).to(d), True), (wide_t[:, :H], True)):
        out = torch.full((n,), -7.0, dtype=torch.float64, device=d)
        N.group_norms(W0, transposed, H, col0, n, out)
        got = out.cpu().numpy()
        assert (np.abs(got - want) <= H * 2.0 ** -52 * want).all() and got[3] == 0.0 and want.max() > 0
    # errors: H < 1, n < 0, ld shorter than the row, out misaligned, out inside W0
    lib = N.lib()
    W0 = torch.from_numpy(W).to(d)
    out = torch.zeros(n + 1, dtype=torch.float64, device=d)
    for args, code in (((W0.data_ptr(), D, 0, 0, col0, n, out.data_ptr()), -1),
                       ((W0.data_ptr(), D, 0, H, col0, -1, out.data_ptr()), -1),
                       ((W0.data_ptr(), col0 + n - 1, 0, H, col0, n, out.data_ptr()), -1),
                       ((W0.data_ptr(), H - 1, 1, H, col0, n, out.data_ptr()), -1),
                       ((W0.data_ptr(), D, 2, H, col0, n, out.data_ptr()), -1),
                       ((None, D, 0, H, col0, n, out.data_ptr()), -1),
                       ((W0.data_ptr(), D, 0, H, col0, n, out.data_ptr() + 4), -3)):
        assert lib.stdadk_group_norms_f32(*args, None) == code, args[1:6]
    assert lib.stdadk_group_norms_f32(W0.data_ptr(), D, 0, H, col0, n, W0.data_ptr(), None) == -1
    assert lib.stdadk_group_norms_f32(W0.data_ptr(), D, 0, H, col0, 0, None, None) == 0


@pytest.mark.parametrize("basis", bc.BASES)
def test_tie_to_the_models_own_basis(basis):
    """Per-knot SPHI (w = 1, default rho) on the `default227` knot table against the column sums of the float32 phi block
    the materialising feature builder makes for the same sites, within 4x the worst relative gap the float32 ORACLE
    features show against the float64 restatement (basis_diag_achieved.json).  Knots with a site within float32 rounding
    of their support edge are left out of this one check (at most 2 % of them).  The column sums run over the pairs the
    contract holds in support: for the Gaussian kind the tail beyond rho is dropped by contract (the compact kinds are
    0 there anyway)."""
    from stnf import _native as N
    d = T.dev()
    case = bc.tie_case(basis)
    Ks, S = case["centers"].shape[0], case["coords"].shape[0]
    phi = torch.empty(S, Ks, device=d)
    N.rbf_build(torch.from_numpy(case["coords"]).to(d), None, None, torch.from_numpy(case["centers"]).to(d),
                torch.from_numpy(case["bw"]).to(d), basis, None, None, phi)
    sphi = run(case)[0].cpu().numpy()[:, bc.K_SPHI]
    edge = bc.tie_edge_knots(case)
    assert edge.sum() <= 0.02 * Ks
    gap = bc.tie_gap(bc.tie_column_sums(phi.cpu().numpy(), case), sphi, edge)
    tol = 4.0 * bc.achieved()["tie_oracle_gap"][basis]
    print(f"{basis}: worst relative gap {gap:.3e}, tolerance {tol:.3e}, {int(edge.sum())} edge knots left out")
    assert gap <= tol and (sphi > 0).sum() > 0.9 * Ks


def _trained(d, steps=4):
    """A learnable model after a few TrainStep steps, its initial copy, and a field."""
    from stnf.engine import TrainStep
    from stnf.models import STInterpMLP
    torch.manual_seed(11)
    m = STInterpMLP(p=0, k_spatial_centers=[25, 81, 121], k_temporal_centers=[10, 15], hidden_dims=[128, 64], dropout=0.0,
                    spatial_learnable=True).to(d)
    initial = copy.deepcopy(m)
    rs = np.random.RandomState(3)
    S, nT = 150, 8
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = (np.sin(6 * coords[:, 0])[None, :] + 0.1 * rs.standard_normal((nT, S))).astype(np.float32)
    code = rs.randint(1, 4, size=(nT, S))
    ti, si = np.nonzero(code == 1)
    c = torch.from_numpy(coords[si]).to(d)
    t = torch.from_numpy((ti / (nT - 1)).astype(np.float32)).to(d)
    y = torch.from_numpy(z[ti, si][:, None]).to(d)
    eng = TrainStep(m.train(), lr=5e-2, max_batch=len(si), ema_decay=None, basis_lr_ratio=1.0)
    for _ in range(steps):
        eng.step(None, c, t, y)
    torch.cuda.synchronize()
    return m.eval(), initial, coords, z, [code == k for k in (1, 2, 3)]


def _on_host(m):
    """The same model on the host: a fresh one that loads the state read back."""
    from stnf.models import STInterpMLP
    h = STInterpMLP(p=0, k_spatial_centers=[25, 81, 121], k_temporal_centers=[10, 15], hidden_dims=[128, 64], dropout=0.0,
                    spatial_learnable=True)
    h.load_state_dict({k: a.detach().cpu().clone() for k, a in m.state_dict().items()})
    return h.eval()


def test_end_to_end_on_a_trained_learnable_model():
    """Predictor.basis_diagnostics equals the host route on the tables read back: every exact slot equal, every sum by
    the comparator; the centres moved; grid_scores' `basis` entry carries the same arrays."""
    from stnf.engine import Predictor
    from stnf.utils import basis_diag as BD
    from stnf.utils import basis_diagnostics, grid_scores
    d = T.dev()
    m, initial, coords, z, masks = _trained(d)
    w = masks[0].sum(axis=0).astype(np.float64)
    v = np.linspace(0, 1, len(coords)) ** 2
    v[::9] = np.nan
    raw = Predictor(m).basis_diagnostics(torch.from_numpy(coords).to(d), torch.from_numpy(w).to(d),
                                         torch.from_numpy(v).to(d))
    centers = m.spatial_basis.centers.detach().cpu().numpy()
    bw = m.spatial_basis.bandwidths.detach().cpu().numpy()
    assert np.array_equal(raw["centers"], centers) and np.array_equal(raw["bandwidths"], bw) and raw["rho"] == 1.0
    case = dict(centers=centers, bw=bw, basis="wendland", sizes=(25, 81, 121), coords=coords, w=w, v=v, rho=1.0)
    rk, rsite, aux = bc.restate_longdouble(case)
    assert not bc.compare(raw["knot_acc"], raw["site_acc"], rk, rsite, aux)[0]
    hk, hs = BD.basis_diag_sums_host(*bc.call_args(case))
    for a, b, slots in ((raw["knot_acc"], hk, [bc.K_N, bc.K_NEAR2]), (raw["site_acc"], hs, [bc.S_COVER, bc.S_NEAR2])):
        assert np.array_equal(a[..., slots], b[..., slots])
    # the first layer as the engine stores it (either layout) against the weight read back
    W0 = m._body[0].weight.detach().cpu().numpy()
    want = BD.group_sumsq_host(W0, 0, m.k_spatial + m.k_temporal)
    assert (np.abs(raw["sumsq"] - want) <= W0.shape[0] * 2.0 ** -52 * want).all() and want.min() > 0
    # the public route carries the device's arrays, and equals the host summaries of the tables READ BACK (a host copy of
    # the model takes exp(log_bandwidths) with the host's float32 exp, which may differ from the device's in the last bit:
    # it answers with the same keys, and with the same host-only entries)
    diag = basis_diagnostics(m, coords, train_mask=masks[0], model_initial=initial, site_value=v)
    back = BD.summarize(hk, hs, (25, 81, 121), centers, bw)
    for k in ("knot_count", "site_cover", "dead", "uncovered", "level_dead", "level_uncovered", "knot_nearest",
              "site_nearest", "out_of_domain", "level_bw_mean", "level_bw_std", "knot_weight"):
        assert np.array_equal(np.asarray(diag[k]), np.asarray(back[k])), k
    for k, slot in (("knot_sphi", bc.K_SPHI), ("knot_sphi2", bc.K_SPHI2), ("knot_weight", bc.K_W)):
        assert np.array_equal(diag[k], raw["knot_acc"][:, slot]), k
    assert np.array_equal(diag["site_sphi"], raw["site_acc"][:, :, bc.S_SPHI])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = raw["knot_acc"][:, bc.K_SV] / raw["knot_acc"][:, bc.K_WV]
    assert np.array_equal(diag["knot_value"], ratio, equal_nan=True)
    assert np.allclose(diag["sparsity_norms"], np.sqrt(want[:m.k_spatial]), rtol=1e-12, atol=0)
    assert np.allclose(diag["temporal_sparsity_norms"], np.sqrt(want[m.k_spatial:]), rtol=1e-12, atol=0)
    host = basis_diagnostics(_on_host(m), coords, train_mask=masks[0], model_initial=_on_host(initial), site_value=v)
    assert set(diag) == set(host)
    for k in ("movement", "path_length", "out_of_domain", "temporal_support", "site_weight", "level_sizes"):
        assert np.array_equal(np.asarray(diag[k]), np.asarray(host[k])), k
    assert np.array_equal(diag["movement"], np.linalg.norm(
        centers.astype(np.float64) - initial.spatial_basis.centers.detach().cpu().numpy().astype(np.float64), axis=1))
    assert np.array_equal(diag["knot_count"], rk[:, bc.K_N].astype(np.int64))
    assert diag["movement_max"] > 0 and (diag["movement"] > 0).sum() > 100
    # grid_scores: the same arrays under `basis`, nothing else changed
    plain = grid_scores(m, z, coords, *masks)
    got = grid_scores(m, z, coords, *masks, config={"basis_diagnostics": True})
    assert set(got) == set(plain) | {"basis"}
    np.testing.assert_equal({k: a for k, a in got.items() if k != "basis"}, plain)
    again = Predictor(m).basis_diagnostics(torch.from_numpy(coords).to(d), torch.from_numpy(w).to(d),
                                           torch.from_numpy(plain["site_mse_by_split"][3]).to(d))["knot_acc"]
    assert np.array_equal(got["basis"]["knot_count"], diag["knot_count"])
    assert np.array_equal(got["basis"]["site_cover"], diag["site_cover"])
    assert np.array_equal(got["basis"]["knot_sphi"], diag["knot_sphi"])
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(got["basis"]["knot_value"], again[:, bc.K_SV] / again[:, bc.K_WV], equal_nan=True)
    assert np.isfinite(got["basis"]["knot_value"]).sum() > 100
