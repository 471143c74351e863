"""Empirical space-time variograms on the device: stdadk_variogram_f32 through the ABI on the generated cases of
tests/golden/variogram_cases.py against its exact restatement -- every N EXACT, every sum within N 2^-52 of the
reference, every slot compared -- at S around every tile edge, nT and lags around each other, 1 / 5 / 64 bins; the pair
rule on the diagonal, the half-open bins, validity, the arguments, determinism and every error code; one mid-size case
against the vectorised restatement; then end to end: Predictor.variogram_grid against the restatement of predict_grid's
own output, grid_scores' `variogram` entry and field_variogram."""
import ctypes as C

import numpy as np
import pytest
import torch

from golden import variogram_cases as vc
import test_gpu_parity as T

pytestmark = pytest.mark.gpu


def run(y, col, z, code, coords, e2, L, fill=-7.0):
    """One call on a pre-filled accumulator (it is ASSIGNED); returns the device tensor."""
    from stnf import _native as N
    d = T.dev()
    nT, S = z.shape
    B = len(e2) - 1
    acc = torch.full((4, L, B, 4), fill, dtype=torch.float64, device=d)
    ws = torch.empty(N.variogram_workspace_bytes(S, nT, B, L) // 8, dtype=torch.float64, device=d)
    N.variogram(None if y is None else torch.from_numpy(y).to(d), col, torch.from_numpy(z).to(d),
                None if code is None else torch.from_numpy(code).to(d), torch.from_numpy(coords).to(d), e2, L, acc, ws)
    return acc


@pytest.mark.parametrize("S", vc.SIZES)
def test_kernel_matches_exact_restatement(S):
    """nT in {1, 2, 7} x lags in {1, 2, 7, 9}; bins 1 / 5 / 64, split NULL and given, y_pred NULL / ldy 5 col 4 / ldy 5
    col 0 / ldy 1, edges2[0] = 0 and > 0 cycle along the runs (variogram_cases.toggles); the edges sit on attained
    values of d2 and the last one below the largest, sites are duplicated."""
    runs = []
    k = vc.SIZES.index(S)
    for nT in vc.SLICES:
        for L in vc.LAGS:
            split_given, pred, first_zero = vc.toggles(k)
            B = vc.BINS[k % 3]
            y, z, code, coords = vc.make_case(S, nT, seed=k, ldy=pred[0] if pred else 1, spread=8 if S < 40 else 32)
            code = code if split_given else None
            e2 = vc.edges_on_attained(coords, B, first_zero)
            col = pred[1] if pred else 0
            runs.append((nT, L, B, pred, None if pred is None else y[:, col].reshape(nT, S), z, code, coords, e2,
                         run(y if pred else None, col, z, code, coords, e2, L)))
            k += 1
    pairs = 0
    for nT, L, B, pred, p, z, code, coords, e2, acc in runs:         # (the launches are all queued before the reads)
        got = acc.cpu().numpy()
        ref = vc.restate_exact(p, z, code, coords, e2, L)
        bad = vc.compare(got, ref)
        assert not bad, (S, nT, L, B, pred, bad[:5])
        if pred is None:
            assert not got[..., vc.SP:].any()
        pairs += int(ref[..., vc.N_].sum())
    assert pairs > 0 or S == 1
    print(f"S={S}: {len(runs)} runs, {pairs} counted pair-slices")


def test_the_diagonal_is_the_only_difference():
    """A field that does not change from slice 0 to slice 1: lag 0 over both slices takes every unordered pair twice,
    lag 1 takes both orders of it once -- the same terms (dyadic values: the sums are exact in any order) -- plus the
    pairs i = j, which add their count to the bin of d2 = 0 and nothing to the sums.  With edges2[0] > 0 the two lags
    agree in every slot.  One tile against itself (S = 16), and ragged tiles (S = 40)."""
    for S in (vc.TILE, 40):
        y, z, code, coords = vc.make_case(S, 1, seed=21, spread=8)
        y2, z2, code2 = np.concatenate([y, y]), np.concatenate([z, z]), np.concatenate([code, code])
        counted = vc._codes(z, code)[0]
        for first_zero in (True, False):
            e2 = vc.edges_on_attained(coords, 5, first_zero)
            got = run(y2, 0, z2, code2, coords, e2, 2).cpu().numpy()
            assert not vc.compare(got, vc.restate_exact(y2[:, 0].reshape(2, S), z2, code2, coords, e2, 2))
            diff = got[:, 1] - got[:, 0]
            want = np.zeros_like(diff)
            if first_zero:
                want[:, 0, vc.N_] = [(counted == c).sum() for c in range(4)]
            assert np.array_equal(diff, want) and got[:, 0, :, vc.N_].sum() > 0


def test_half_open_bins_on_a_line():
    """Nine sites an eighth apart, every entry counted, z = the site's index: separations k / 8 occur 9 - k times.
    edges2 = (1/8)^2, (3/8)^2, (5/8)^2: bin 0 holds k = 1, 2 (the lower edge is in), bin 1 k = 3, 4 (the upper edge is
    out of bin 0), k = 0 and k >= 5 count nowhere."""
    S = 9
    coords = np.stack([np.arange(S) / 8.0, np.zeros(S)], axis=1).astype(np.float32)
    z = np.arange(S, dtype=np.float32)[None, :].repeat(2, axis=0)
    e2 = np.array([1, 9, 25]) / 64.0
    got = run(None, 0, z, None, coords, e2, 2).cpu().numpy()
    # lag 0, two slices: N = 2 (9 - k) per k, SZ = k^2 each; lag 1, one slice, both orders: the same numbers
    for u in (0, 1):
        assert got[0, u, 0].tolist() == [2 * (8 + 7), 2 * (8 * 1 + 7 * 4), 0, 0]
        assert got[0, u, 1].tolist() == [2 * (6 + 5), 2 * (6 * 9 + 5 * 16), 0, 0]
    assert not got[1:].any()


def test_validity():
    """No counted entry: zeros.  Pairs across splits count nowhere.  NaN and +-inf entries and code 7 count nowhere."""
    S, nT = 33, 3
    y, z, code, coords = vc.make_case(S, nT, seed=31, spread=8)
    e2 = vc.edges_on_attained(coords, 5)
    assert not run(y, 0, np.full_like(z, np.nan), code, coords, e2, 3).cpu().numpy().any()
    assert not run(y, 0, z, np.full_like(code, 7), coords, e2, 3).cpu().numpy().any()
    zz = np.ones((nT, 2), dtype=np.float32)
    two = np.array([[0, 0], [0.125, 0]], dtype=np.float32)
    cross = run(None, 0, zz, np.array([[1, 2]] * nT, dtype=np.uint8), two, np.array([0.0, 1.0]), 1).cpu().numpy()
    same = run(None, 0, zz, np.array([[2, 2]] * nT, dtype=np.uint8), two, np.array([0.0, 1.0]), 1).cpu().numpy()
    assert not cross.any() and same[2, 0, 0].tolist() == [nT, 0, 0, 0] and same.sum() == nT
    bad = z.copy()
    bad[0, :3] = [np.nan, np.inf, -np.inf]
    code[1, 4] = 7
    got = run(y, 0, bad, code, coords, e2, 3).cpu().numpy()
    assert not vc.compare(got, vc.restate_exact(y[:, 0].reshape(nT, S), bad, code, coords, e2, 3))
    # S = 0 and nT = 0: zeros
    for shape in ((3, 0), (0, 5)):
        acc = run(None, 0, np.zeros(shape, dtype=np.float32), None, np.zeros((shape[1], 2), dtype=np.float32), e2, 2)
        assert not acc.cpu().numpy().any()


def test_prediction_null_and_columns():
    """y_pred NULL: SP = SR = 0, N and SZ the bits of the call with one; ldy = 5 with col = 4 and col = 0 read their own
    column."""
    S, nT, L = 65, 7, 3
    y, z, code, coords = vc.make_case(S, nT, seed=41, ldy=5)
    e2 = vc.edges_on_attained(coords, 5)
    none = run(None, 0, z, code, coords, e2, L).cpu().numpy()
    cols = {col: run(y, col, z, code, coords, e2, L).cpu().numpy() for col in (0, 4)}
    alone = run(np.ascontiguousarray(y[:, 4:5]), 0, z, code, coords, e2, L).cpu().numpy()
    assert not none[..., vc.SP:].any() and none[..., vc.SZ].sum() > 0
    for col, got in cols.items():
        assert np.array_equal(got[..., :vc.SP], none[..., :vc.SP])
        assert not vc.compare(got, vc.restate_exact(y[:, col].reshape(nT, S), z, code, coords, e2, L))
    assert np.array_equal(cols[4], alone) and not np.array_equal(cols[0], cols[4])


def test_same_call_same_bits():
    rs = np.random.RandomState(5)
    S, nT, L = 257, 7, 3
    coords = rs.uniform(size=(S, 2)).astype(np.float32)
    z = rs.standard_normal((nT, S)).astype(np.float32)
    y = rs.standard_normal((nT * S, 3)).astype(np.float32)
    code = rs.randint(0, 4, size=(nT, S)).astype(np.uint8)
    e2 = np.linspace(0, 0.7, 16) ** 2
    a = run(y, 1, z, code, coords, e2, L, fill=-7.0).cpu().numpy()
    b = run(y, 1, z, code, coords, e2, L, fill=3.0).cpu().numpy()
    assert np.array_equal(a, b) and a[..., vc.N_].sum() > 0


def _raw(d, S=20, nT=3, B=4, L=2, ldy=2, col=0, edges=None, acc_off=0, ws_off=0, ws_short=0, alias=None, pred=True):
    """The C call itself with one thing wrong; returns (code, everything the call could have written)."""
    from stnf import _native as N
    rows = max(S * nT, 1) if S * nT < 2 ** 31 else 1
    y = torch.zeros(rows, ldy, device=d)
    z, coords = torch.zeros(rows, device=d), torch.zeros(max(S, 1) if S < 2 ** 20 else 1, 2, device=d)
    need = N.lib().stdadk_variogram_workspace_bytes(S, nT, B, L)
    acc = torch.full((4 * max(L, 1) * max(B, 1) * 4 + 2,), 3.0, dtype=torch.float64, device=d)
    ws = torch.full((need // 8 + 2,), 3.0, dtype=torch.float64, device=d)
    e = np.linspace(0, 1, max(B, 1) + 1) if edges is None else np.asarray(edges, dtype=np.float64)
    acc_p = {"z": z.data_ptr(), "ws": ws.data_ptr(), None: acc.data_ptr() + acc_off}[alias]
    rc = N.lib().stdadk_variogram_f32(y.data_ptr() if pred else None, ldy, col, z.data_ptr(), None, coords.data_ptr(), S,
                                      nT, (C.c_double * len(e))(*e), B, L, acc_p, ws.data_ptr() + ws_off,
                                      need - ws_short, None)
    torch.cuda.synchronize()
    return rc, bool((acc == 3.0).all()) and bool((ws == 3.0).all())


@pytest.mark.parametrize("what,kw,code", [
    ("n_bins 0", dict(B=0), -1), ("n_bins 65", dict(B=65), -1), ("n_lags 0", dict(L=0), -1), ("n_lags 17", dict(L=17), -1),
    ("edges not increasing", dict(edges=[0, 0.5, 0.5, 0.7, 1]), -1), ("edges decreasing", dict(edges=[0, 0.5, 0.4, 0.7, 1]), -1),
    ("edges2[0] < 0", dict(edges=[-0.1, 0.5, 0.6, 0.7, 1]), -1), ("col = ldy", dict(col=2), -1), ("col < 0", dict(col=-1), -1),
    ("S nT = 2^31", dict(S=2 ** 16, nT=2 ** 15), -2), ("acc misaligned", dict(acc_off=4), -3),
    ("workspace misaligned", dict(ws_off=4), -3), ("workspace short", dict(ws_short=8), -4),
    ("acc aliases z", dict(alias="z"), -1), ("acc aliases the workspace", dict(alias="ws"), -1)])
def test_every_error_code(what, kw, code):
    from stnf import _native as N
    assert (N.lib().stdadk_variogram_workspace_bytes(2 ** 16, 2 ** 15, 4, 2), N.lib().stdadk_variogram_workspace_bytes(5, 5, 0, 1),
            N.lib().stdadk_variogram_workspace_bytes(5, 5, 4, 17)) == (0, 0, 0)
    rc, untouched = _raw(T.dev(), **kw)
    assert rc == code and untouched, (what, rc, N.lib().stdadk_last_error())
    # col is not looked at without a prediction, and the good call succeeds
    assert _raw(T.dev(), col=7, pred=False)[0] == 0 and _raw(T.dev())[0] == 0


def test_mid_size_against_the_vectorised_restatement():
    """S = 700, nT = 20, 3 lags, 15 bins of equal width, ordinary float32 values (nothing dyadic: the sums round) with
    NaNs and mixed codes: N exact, sums within 2 N 2^-52 (the reference is itself a numpy sum)."""
    rs = np.random.RandomState(9)
    S, nT, L = 700, 20, 3
    coords = rs.uniform(size=(S, 2)).astype(np.float32)
    z = rs.standard_normal((nT, S)).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.1] = np.nan
    y = (0.8 * z + 0.3 * rs.standard_normal((nT, S)).astype(np.float32)).reshape(-1, 1)
    y = np.where(np.isfinite(y), y, 0).astype(np.float32)
    code = np.where(rs.uniform(size=z.shape) < 0.05, 7, rs.randint(0, 4, size=z.shape)).astype(np.uint8)
    e2 = np.linspace(0, 0.7, 16) ** 2
    acc = run(y, 0, z, code, coords, e2, L)
    ref = vc.restate_numpy(y.reshape(nT, S), z, code, coords, e2, L)
    got = acc.cpu().numpy()
    bad = vc.compare(got, ref, factor=2.0)
    assert not bad, bad[:5]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - ref)[..., 1:] / (2 * ref[..., :1] * 2.0 ** -52 * np.abs(ref[..., 1:]))
    print(f"mid-size: {int(ref[..., vc.N_].sum())} pair-slices, worst |delta| / bound = {np.nanmax(r):.4f}")
    assert ref[..., vc.N_].min() > 0


# ------------------------------------------------------------------------------------------------ end to end
def _field(d):
    coords, z, code = vc.e2e_field()
    tv = vc.grid_times(vc.E2E_T)
    return coords, z, code, tuple(torch.from_numpy(a).to(d) for a in (coords, tv, z, code))


def test_variogram_grid_equals_restatement_of_predict_grid():
    """All sites and an index array, the default column (the median) and another, edges given and by default."""
    from stnf.engine import Predictor
    d = T.dev()
    m = vc.e2e_model().to(d)
    coords, z, code, (ct, tvt, zt, codet) = _field(d)
    pr = Predictor(m, chunk=4096)
    c64 = coords.astype(np.float64)
    dflt = np.linspace(0, 0.5 * np.hypot(*(c64.max(axis=0) - c64.min(axis=0))), 16)
    for sites, col, kw, edges, L in ((None, 1, {}, dflt, 1),
                                     (np.arange(1, vc.E2E_S, 3), 2, dict(metric_col=2, n_bins=6, max_dist=0.5, time_lags=4),
                                      np.linspace(0, 0.5, 7), 4),
                                     ("all", 0, dict(metric_col=0, edges=[0.05, 0.2, 0.9], time_lags=2), [0.05, 0.2, 0.9], 2)):
        out = pr.variogram_grid(ct, tvt, zt, codet, sites=sites, **kw)
        idx = np.arange(vc.E2E_S) if sites is None or isinstance(sites, str) else sites
        assert np.array_equal(out["sites"], idx) and np.array_equal(out["edges"], np.asarray(edges, dtype=np.float64))
        e2 = np.asarray(edges, dtype=np.float64) ** 2
        grid = pr.predict_grid(ct[torch.from_numpy(idx).to(d)].contiguous(), tvt).cpu().numpy()       # (T, S', Q)
        ref = vc.restate_exact(grid[:, :, col], z[:, idx], code[:, idx], coords[idx], e2, L)
        bad = vc.compare(out["acc"], ref)
        assert not bad, (col, bad[:5])
        assert ref[..., vc.N_].sum() > 0 and np.array_equal(out["count"], ref[..., vc.N_])
        with np.errstate(divide="ignore", invalid="ignore"):
            want = ref[..., vc.SR] / (2 * ref[..., vc.N_])
        assert np.allclose(out["gamma_resid"], want, rtol=1e-12, atol=0, equal_nan=True)
        assert out["lags"].tolist() == list(range(L))
    with pytest.raises(ValueError):
        pr.variogram_grid(ct, tvt, zt, codet, metric_col=3)


def test_grid_scores_variogram_entry():
    """With `variogram: true` the entry is the restatement of the device's own grid, divided; without the key the keys
    and values are what they are without the feature."""
    from stnf.engine import Predictor
    from stnf.utils import grid_scores
    from stnf.utils.predictions import SPLIT_NAMES
    d = T.dev()
    m = vc.e2e_model().to(d)
    coords, z, code, (ct, tvt, _, _) = _field(d)
    masks = [code == c for c in (1, 2, 3)]
    config = {"regression_type": "multi-quantile", "quantile_levels": [0.1, 0.5, 0.9]}
    plain = grid_scores(m, z, coords, *masks, config=config)
    assert "variogram" not in plain
    got = grid_scores(m, z, coords, *masks, config=dict(config, variogram=True, variogram_bins=6,
                                                         variogram_max_dist=0.5, variogram_time_lags=3))
    assert set(got) == set(plain) | {"variogram"}
    np.testing.assert_equal({k: v for k, v in got.items() if k != "variogram"}, plain)
    grid = Predictor(m).predict_grid(ct, tvt).cpu().numpy()
    edges = np.linspace(0, 0.5, 7)
    ref = vc.restate_exact(grid[:, :, 1], z, code, coords, edges * edges, 3)
    for c, name in enumerate(SPLIT_NAMES):
        e = got["variogram"][name]
        assert np.array_equal(e["count"], ref[c, :, :, vc.N_]) and e["count"].sum() > 0
        for key, slot in (("gamma_z", vc.SZ), ("gamma_pred", vc.SP), ("gamma_resid", vc.SR)):
            with np.errstate(divide="ignore", invalid="ignore"):
                want = ref[c, :, :, slot] / (2 * ref[c, :, :, vc.N_])
            assert np.allclose(e[key], want, rtol=1e-12, atol=0, equal_nan=True), (name, key)
        assert np.array_equal(e["edges"], edges) and e["lags"].tolist() == [0, 1, 2]


def test_field_variogram_is_the_call_without_a_prediction():
    from stnf.utils import field_variogram
    d = T.dev()
    coords, z, code, (ct, tvt, zt, codet) = _field(d)
    out = field_variogram(zt, coords, code, n_bins=6, max_dist=0.5, time_lags=3)
    e2 = np.linspace(0, 0.5, 7) ** 2
    acc = run(None, 0, z, code, coords, e2, 3).cpu().numpy()
    assert np.array_equal(out["count"], acc[..., vc.N_]) and out["count"].sum() > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(out["gamma_z"], np.where(acc[..., 0] > 0, acc[..., vc.SZ] / (2 * acc[..., 0]), np.nan),
                              equal_nan=True)
    assert not vc.compare(acc, vc.restate_exact(None, z, code, coords, e2, 3))
    host = field_variogram(z, coords, code, n_bins=6, max_dist=0.5, time_lags=3)
    assert np.array_equal(host["count"], out["count"])
    assert np.allclose(host["gamma_z"], out["gamma_z"], rtol=1e-12, atol=0, equal_nan=True)
