"""Local ordinary kriging on the device: stdadk_krige_weights_f64 and stdadk_krige_apply_f32 through the ABI on every
generated case of tests/golden/kriging_cases.py, on pre-filled outputs -- with the spherical model (and on the exactly
singular case) w and var BIT-EQUAL to kriging_weights_host, NaN positions included; with the exponential and gaussian
models, which go through the device's exp, within K_exp kappa 2^-52 max|w| per row, K_exp as measured on the host
(tests/golden/kriging_achieved.json) and kappa <= 1e9 by the generator; the apply bit-equal to kriging_apply_host given
the device's own weights -- determinism, empty sides, every error code with everything writable left untouched, a
captured graph; then grid_baselines with `baseline_kriging` on the device against the host route, and grid_scores'
`baseline` entry with it on a small trained model."""
import json
import os

import numpy as np
import pytest
import torch

from golden import kriging_cases as kc
import test_gpu_parity as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZQ4 = [-1.2815515655446004, 0.0, 0.6744897501960817, 1.6448536269514722]


def _to(d, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(d)


def k_exp():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "kriging_achieved.json")))["K_exp"]


def weights(case, tab, fill=-7.0):
    """One call on pre-filled outputs (both are ASSIGNED); returns the device tensors (idx, w, var)."""
    from stnf import _native as N
    from stnf.utils import kriging as KR
    d = T.dev()
    idx, d2 = _to(d, tab[0]), _to(d, tab[1])
    nM, M, _ = idx.shape
    w = torch.full((nM, M, case["k"]), fill, dtype=torch.float64, device=d)
    var = torch.full((nM, M), fill, dtype=torch.float64, device=d)
    N.krige_weights(idx, d2, case["k"], _to(d, case["coords"]), KR.model_code(case["model"]), case["nugget"], case["psill"],
                    case["range"], w, var)
    return idx, w, var


def apply(idx, w, var, k, z, zq, ldo=None, fill=-7.0):
    from stnf import _native as N
    out = torch.full((z.shape[0] * idx.shape[1], ldo or len(zq)), fill, dtype=torch.float32, device=z.device)
    N.krige_apply(idx, w, var, k, z, zq, out)
    return out


@pytest.fixture(scope="module")
def hosted():
    """(case, table, kriging_weights_host's (w, var)) of every generated case: computed once, never changed."""
    from stnf.utils import kriging as KR
    out = []
    for case in kc.all_cases():
        tab = kc.table(case)
        out.append((case, tab, KR.kriging_weights_host(tab[0], tab[1], case["k"], case["coords"], case["model"],
                                                       case["nugget"], case["psill"], case["range"])))
    return out


def test_weights_and_apply_against_the_host_statements_on_every_case(hosted):
    from stnf.utils import kriging as KR
    d = T.dev()
    outs = [weights(case, tab) for case, tab, _ in hosted]       # (the launches are all queued before the reads)
    n_bit = len(kc.bitwise_cases())
    bit_rows = bound_rows = values = 0
    worst = 0.0
    for n, ((case, tab, (hw, hvar)), (idx, w, var)) in enumerate(zip(hosted, outs)):
        what = (case["model"], len(case["q"]), case["k"], case["nugget"], case["range"])
        gw, gvar = w.cpu().numpy(), var.cpu().numpy()
        if n < n_bit:
            assert kc.same_bits(gw, hw) and kc.same_bits(gvar, hvar), what
            bit_rows += gvar.size
        else:
            kappa = kc.reference(case, tab)[2]
            ok, ratio = kc.within_exp_bound(gw, gvar, hw, hvar, kappa, k_exp(), case["nugget"] + case["psill"])
            print(what, f"worst |w - w_host| / (kappa 2^-52 max|w|) = {ratio * k_exp():.3g} (allowed {k_exp():.3g})")
            assert ok, what + (ratio,)
            worst, bound_rows = max(worst, ratio), bound_rows + gvar.size
        z = _to(d, case["z"])
        for zq, ldo in (([0.0], None), (ZQ4, None), (ZQ4, 6)):
            out = apply(idx, w, var, case["k"], z, zq, ldo).cpu().numpy()
            want = KR.kriging_apply_host(tab[0], gw, gvar, case["k"], case["z"], zq).reshape(-1, len(zq))
            assert kc.same_bits(out[:, :len(zq)], want), what + (len(zq), ldo)
            assert (out[:, len(zq):] == -7.0).all()                      # the columns beyond Q are not written
            values += int(np.isfinite(want).sum())
    print(f"{bit_rows} rows bit-equal, {bound_rows} rows within the exp bound (worst {worst:.3g} of it), "
          f"{values} predictions bit-equal")
    assert bit_rows > 1000 and bound_rows > 900 and values > 20000


def test_same_call_same_bits(hosted):
    case, tab, _ = next(h for h in hosted if h[0]["k"] == 16 and h[0]["model"] == "exponential")
    a, b = weights(case, tab, fill=-7.0), weights(case, tab, fill=3.0)
    assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)) and torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
    z = _to(T.dev(), case["z"])
    assert torch.equal(apply(*a, 16, z, ZQ4).view(torch.int32), apply(*b, 16, z, ZQ4, fill=3.0).view(torch.int32))


def test_empty_sides():
    """M = 0 or nM = 0 writes nothing; a table of -1 (S = 0, or a slice without sources) gives w = 0 and var = NaN,
    and NaN predictions; nT = 0 is no call."""
    from stnf import _native as N
    d = T.dev()
    coords = torch.zeros(5, 2, device=d)
    for shape in ((1, 0, 8), (0, 7, 8)):
        idx, d2 = torch.zeros(shape, dtype=torch.int32, device=d), torch.zeros(shape, dtype=torch.float64, device=d)
        w, var = torch.zeros(shape[:2] + (4,), dtype=torch.float64, device=d), torch.zeros(shape[:2], dtype=torch.float64, device=d)
        N.krige_weights(idx, d2, 4, coords, 0, 0.1, 1.0, 0.5, w, var)
    idx = torch.full((2, 70, 8), -1, dtype=torch.int32, device=d)
    d2 = torch.full((2, 70, 8), float("inf"), dtype=torch.float64, device=d)
    w, var = torch.full((2, 70, 8), -7.0, dtype=torch.float64, device=d), torch.full((2, 70), -7.0, dtype=torch.float64, device=d)
    N.krige_weights(idx, d2, 8, coords[:0], 2, 0.0, 1.0, 0.5, w, var)
    assert bool((w == 0).all()) and bool(torch.isnan(var).all())
    out = apply(idx, w, var, 8, torch.zeros(2, 0, device=d), [0.0, 1.0])
    assert out.shape == (140, 2) and bool(torch.isnan(out).all())
    out = apply(idx[:1], w[:1], var[:1], 8, torch.zeros(0, 0, device=d), [0.0])
    assert out.shape == (0, 1)
    idx[:, :, 0] = 9                                             # an index >= S is never dereferenced
    N.krige_weights(idx, d2, 8, coords, 1, 0.1, 1.0, 0.5, w, var)
    assert bool((w == 0).all()) and bool(torch.isnan(var).all())


def _raw(d, nM=1, M=70, k_tab=8, k=8, S=300, model=0, nugget=0.1, psill=1.0, range_=0.5, idx_off=0, d2_off=0, w_off=0,
         var_off=0, coords_off=0, alias=None, null=()):
    """The C weights call itself with one thing wrong; returns (code, whether everything writable is untouched)."""
    from stnf import _native as N
    lib = N.lib()
    ok = lambda n: n if 0 < n < 2 ** 20 else 1                   # noqa: E731  (a refused size is never indexed)
    nm, nq, ns, kt = ok(nM), ok(M), ok(S), k_tab if 0 < k_tab <= 16 else 1
    idx = torch.zeros(nm * nq * kt + 2, dtype=torch.int32, device=d)
    d2 = torch.ones(nm * nq * kt + 2, dtype=torch.float64, device=d)
    coords = torch.zeros(ns + 1, 2, device=d)
    w = torch.full((nm * nq * kt + 2,), 3.0, dtype=torch.float64, device=d)
    var = torch.full((nm * nq + 2,), 3.0, dtype=torch.float64, device=d)
    ptr = {"idx": idx.data_ptr() + idx_off, "d2": d2.data_ptr() + d2_off, "coords": coords.data_ptr() + coords_off,
           "w": w.data_ptr() + w_off, "var": var.data_ptr() + var_off}
    if alias:
        ptr[alias[0]] = ptr[alias[1]]
    for name in null:
        ptr[name] = None
    rc = lib.stdadk_krige_weights_f64(ptr["idx"], ptr["d2"], nM, M, k_tab, k, ptr["coords"], S, model, nugget, psill, range_,
                                      ptr["w"], ptr["var"], None)
    torch.cuda.synchronize()
    return rc, bool((w == 3.0).all()) and bool((var == 3.0).all())


@pytest.mark.parametrize("what,kw,code", [
    ("M < 0", dict(M=-1), -1), ("S = 2^31", dict(S=2 ** 31), -1), ("nM < 0", dict(nM=-1), -1),
    ("model 3", dict(model=3), -1), ("model < 0", dict(model=-1), -1), ("nugget < 0", dict(nugget=-0.1), -1),
    ("psill < 0", dict(psill=-1.0), -1), ("nugget + psill = 0", dict(nugget=0.0, psill=0.0), -1),
    ("range = 0", dict(range_=0.0), -1), ("range < 0", dict(range_=-1.0), -1), ("range NaN", dict(range_=float("nan")), -1),
    ("nugget inf", dict(nugget=float("inf")), -1), ("psill NaN", dict(psill=float("nan")), -1),
    ("k = 0", dict(k=0), -1), ("k > k_tab", dict(k_tab=4, k=5), -1), ("k_tab = 17", dict(k_tab=17, k=1), -1),
    ("NULL nbr_idx", dict(null=("idx",)), -1), ("NULL nbr_d2", dict(null=("d2",)), -1), ("NULL coords", dict(null=("coords",)), -1),
    ("NULL w", dict(null=("w",)), -1), ("NULL var", dict(null=("var",)), -1),
    ("w aliases nbr_d2", dict(alias=("w", "d2")), -1), ("var aliases coords", dict(alias=("var", "coords")), -1),
    ("w aliases var", dict(alias=("w", "var")), -1), ("var aliases nbr_idx", dict(alias=("var", "idx")), -1),
    ("nM*M*k_tab = 2^31", dict(M=2 ** 27, nM=2, k_tab=8), -2), ("nM*M = 2^31", dict(M=2 ** 16, nM=2 ** 15, k_tab=1, k=1), -2),
    ("nbr_d2 misaligned", dict(d2_off=4), -3), ("w misaligned", dict(w_off=4), -3), ("var misaligned", dict(var_off=4), -3),
    ("nbr_idx misaligned", dict(idx_off=2), -3), ("coords misaligned", dict(coords_off=2), -3)])
def test_every_error_code_of_the_weights(what, kw, code):
    from stnf import _native as N
    rc, untouched = _raw(T.dev(), **kw)
    assert rc == code and untouched, (what, rc, N.lib().stdadk_last_error())
    assert _raw(T.dev())[0] == 0 and _raw(T.dev(), nM=3, model=2, nugget=0.0)[0] == 0      # the good calls succeed


def _raw_apply(d, nM=1, M=70, k_tab=8, k=8, nT=3, S=300, Q=2, ldo=2, zq=(0.0, 1.0), idx_off=0, w_off=0, var_off=0, z_off=0,
               out_off=0, alias=None, null=()):
    import ctypes as C
    from stnf import _native as N
    lib = N.lib()
    ok = lambda n: n if 0 < n < 2 ** 20 else 1                   # noqa: E731
    nm, nq, nt, ns, kt = ok(nM), ok(M), ok(nT), ok(S), k_tab if 0 < k_tab <= 16 else 1
    idx = torch.zeros(nm * nq * kt + 2, dtype=torch.int32, device=d)
    w = torch.ones(nm * nq * kt + 2, dtype=torch.float64, device=d)
    var = torch.ones(nm * nq + 2, dtype=torch.float64, device=d)
    z = torch.zeros(nt * ns + 2, device=d)
    out = torch.full((nt * nq * (ldo if 0 < ldo < 64 else 1) + 2,), 3.0, device=d)
    ptr = {"idx": idx.data_ptr() + idx_off, "w": w.data_ptr() + w_off, "var": var.data_ptr() + var_off,
           "z": z.data_ptr() + z_off, "out": out.data_ptr() + out_off, "zq": (C.c_double * 8)(*(list(zq) + [0.0] * (8 - len(zq))))}
    if alias:
        ptr[alias[0]] = ptr[alias[1]]
    for name in null:
        ptr[name] = None
    rc = lib.stdadk_krige_apply_f32(ptr["idx"], ptr["w"], ptr["var"], nM, M, k_tab, k, ptr["z"], nT, S, ptr["zq"], Q, ptr["out"],
                                    ldo, None)
    torch.cuda.synchronize()
    return rc, bool((out == 3.0).all())


@pytest.mark.parametrize("what,kw,code", [
    ("M < 0", dict(M=-1), -1), ("S = 2^31", dict(S=2 ** 31), -1), ("nT < 0", dict(nT=-1), -1),
    ("nM neither 1 nor nT", dict(nM=2), -1), ("k = 0", dict(k=0), -1), ("k > k_tab", dict(k_tab=4, k=5), -1),
    ("k_tab = 17", dict(k_tab=17, k=1), -1), ("Q = 0", dict(Q=0), -1), ("Q = 9", dict(Q=9, ldo=9), -1),
    ("ldo < Q", dict(Q=2, ldo=1), -1), ("zq NULL", dict(null=("zq",)), -1), ("zq not finite", dict(zq=(0.0, float("nan"))), -1),
    ("NULL nbr_idx", dict(null=("idx",)), -1), ("NULL w", dict(null=("w",)), -1), ("NULL var", dict(null=("var",)), -1),
    ("NULL z", dict(null=("z",)), -1), ("NULL out", dict(null=("out",)), -1),
    ("nT*M = 2^31", dict(nT=2 ** 16, M=2 ** 15, S=1), -2), ("nT*S = 2^31", dict(nT=2 ** 16, M=1, S=2 ** 15), -2),
    ("out aliases z", dict(alias=("out", "z")), -1), ("out aliases w", dict(alias=("out", "w")), -1),
    ("out aliases var", dict(alias=("out", "var")), -1), ("out aliases nbr_idx", dict(alias=("out", "idx")), -1),
    ("w misaligned", dict(w_off=4), -3), ("var misaligned", dict(var_off=4), -3), ("nbr_idx misaligned", dict(idx_off=2), -3),
    ("z misaligned", dict(z_off=2), -3), ("out misaligned", dict(out_off=2), -3)])
def test_every_error_code_of_the_apply(what, kw, code):
    from stnf import _native as N
    rc, untouched = _raw_apply(T.dev(), **kw)
    assert rc == code and untouched, (what, rc, N.lib().stdadk_last_error())
    assert _raw_apply(T.dev())[0] == 0 and _raw_apply(T.dev(), nM=3, Q=1, ldo=4)[0] == 0      # the good calls succeed


def test_wrapper_refuses_what_the_neighbouring_wrappers_refuse():
    from stnf import _native as N
    d = T.dev()
    idx, d2 = torch.zeros(1, 5, 3, dtype=torch.int32, device=d), torch.ones(1, 5, 3, dtype=torch.float64, device=d)
    coords = torch.zeros(9, 2, device=d)
    w, var = torch.zeros(1, 5, 2, dtype=torch.float64, device=d), torch.zeros(1, 5, dtype=torch.float64, device=d)
    N.krige_weights(idx, d2, 2, coords, 1, 0.1, 1.0, 0.5, w, var)
    for bad in (dict(idx=idx.long()), dict(d2=d2.float()), dict(coords=coords.double()), dict(coords=coords.cpu()),
                dict(w=w[:, :, :1]), dict(var=var.float()), dict(k=4), dict(model=3), dict(psill=-1.0)):
        a = dict(dict(idx=idx, d2=d2, coords=coords, w=w, var=var, k=2, model=1, psill=1.0), **bad)
        with pytest.raises(RuntimeError):
            N.krige_weights(a["idx"], a["d2"], a["k"], a["coords"], a["model"], 0.1, a["psill"], 0.5, a["w"], a["var"])
    z, out = torch.zeros(3, 9, device=d), torch.zeros(15, 2, device=d)
    N.krige_apply(idx, w, var, 2, z, [0.0, 1.0], out)
    for bad in (dict(z=z.double()), dict(out=out[:10]), dict(out=out[:, :1]), dict(zq=[0.0] * 9), dict(w=w.float())):
        a = dict(dict(z=z, out=out, zq=[0.0, 1.0], w=w), **bad)
        with pytest.raises(RuntimeError):
            N.krige_apply(idx, a["w"], var, 2, a["z"], a["zq"], a["out"])


def test_a_captured_call_replays_the_direct_calls_bytes(hosted):
    from stnf import _native as N
    from stnf.utils import kriging as KR
    d = T.dev()
    case, tab, _ = next(h for h in hosted if h[0]["k"] == 15 and h[0]["src"] is not None)
    idx, w0, var0 = weights(case, tab)
    z, d2, coords = _to(d, case["z"]), _to(d, tab[1]), _to(d, case["coords"])
    out0 = apply(idx, w0, var0, 15, z, ZQ4)
    w, var, out = torch.full_like(w0, -7.0), torch.full_like(var0, -7.0), torch.full_like(out0, -7.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        N.krige_weights(idx, d2, 15, coords, KR.model_code(case["model"]), case["nugget"], case["psill"], case["range"], w, var)
        N.krige_apply(idx, w, var, 15, z, ZQ4, out)
    graph.replay()
    torch.cuda.synchronize()
    same = lambda a, b, t: torch.equal(a.view(t), b.view(t))      # noqa: E731
    assert same(w, w0, torch.int64) and same(var, var0, torch.int64) and same(out, out0, torch.int32)


def _field(T_=7, S=150, seed=4, site_wise=True):
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = (np.sin(5 * coords[:, 0])[None, :] + rs.standard_normal((T_, S)) * 0.2).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.05] = np.nan
    code = np.broadcast_to(rs.randint(1, 4, size=S), (T_, S)) if site_wise else rs.randint(0, 4, size=(T_, S))
    if site_wise:
        z[:, code[0] == 1] = np.where(np.isnan(z[:, code[0] == 1]), 0.5, z[:, code[0] == 1])      # training sites complete
    return coords, z, [code == c for c in (1, 2, 3)]


def _leaves(d, prefix=""):
    for key, v in d.items():
        if isinstance(v, dict):
            yield from _leaves(v, f"{prefix}{key}/")
        else:
            yield prefix + key, v


def _close(got, ref, tol, what):
    """The `kriging` entries of two grid_baselines dicts, leaf by leaf: counts and settings equal, sums within tol."""
    a, b = dict(_leaves(got)), dict(_leaves(ref))
    assert set(a) == set(b), what
    for name, v in b.items():
        g = a[name]
        if isinstance(v, str) or name.endswith(("rows", "n_singular", "bins_used", "/k")) or name in ("k", "model"):
            assert g == v, (what, name, g, v)
        else:
            g, v = np.asarray(g, dtype=np.float64), np.asarray(v, dtype=np.float64)
            assert g.shape == v.shape and np.array_equal(np.isnan(g), np.isnan(v)), (what, name)
            fin = ~np.isnan(v)
            assert (np.abs(g - v)[fin] <= tol * np.maximum(np.abs(v)[fin], 1e-300)).all(), (what, name, g, v)


@pytest.mark.parametrize("site_wise", [True, False])
def test_grid_baselines_with_kriging_on_the_device_equal_the_host_route(site_wise):
    """Spherical: the device's weights and float32 predictions are the host's bit for bit, so both routes score the
    SAME numbers; the sums differ by their order only, within the 1e-12 relative test_gpu_grid_score.py holds
    stdadk_grid_score_f32 to, and a metric is one more rounded operation on top (test_gpu_knn.py's reasoning).
    Exponential: a weight differs by at most K_exp kappa 2^-52 max|w|; with kappa <= 1e4 for nugget / psill = 0.1 at
    k = 8 (K's smallest eigenvalue is at least nugget, its largest at most k psill + nugget) and |w| of order 1 that
    is 3e-11 in a prediction of order 1, under the float32 ulp (6e-8) it is rounded to, except where it crosses a
    rounding boundary: a prediction may move by ONE float32 ulp, 1.2e-7 relative, and an error z - p of the size of the
    noise (0.2) by 6e-7 relative, its square by 1.2e-6; the quantile columns and the variance move alike.  2e-6."""
    from stnf.utils import baselines as BL
    d = T.dev()
    coords, z, masks = _field(site_wise=site_wise)
    for model, tol in (("spherical", 1e-12 + 2.0 ** -52), ("exponential", 2e-6)):
        config = {"baseline_kriging": True, "kriging_model": model, "kriging_params": (0.1, 1.0, 0.4),
                  "kriging_levels": [0.1, 0.9], "kriging_k": 8, "baseline_k": 4}
        for max_rows in (None, 3 * 150):
            host = BL.grid_baselines(z, coords, *masks, config=config, max_rows=max_rows)
            got = BL.grid_baselines(z, coords, *masks, config=config, max_rows=max_rows, device=d)
            assert got["shared_table"] == site_wise and set(got) == set(host)
            _close(got["kriging"], host["kriging"], tol, (site_wise, model, max_rows))
            _close(got["idw"], host["idw"], 1e-12 + 2.0 ** -52, (site_wise, model, max_rows, "idw"))
    e = got["kriging"]
    assert np.isfinite(e["splits"]["test"]["mse"]) and e["splits"]["test"]["rows"] > 0 and e["n_singular"] == 0
    assert 0.3 < e["splits"]["test"]["coverage"] <= 1.0 and np.isfinite(e["msse"]["test"])
    fitted = BL.grid_baselines(z, coords, *masks, config={"baseline_kriging": True}, device=d)      # the fit on the device
    fit_host = BL.grid_baselines(z, coords, *masks, config={"baseline_kriging": True})
    assert fitted["kriging"]["variogram_fit"]["range"] == fit_host["kriging"]["variogram_fit"]["range"]
    assert fitted["kriging"]["variogram_fit"]["bins_used"] >= 3


def test_grid_scores_baseline_entry_with_kriging_on_a_trained_model():
    """`baseline` gains `kriging`, `skill` its third name and `site_skill` its third row; everything else is
    bit-identical to the call without `baseline_kriging`."""
    from stnf.engine import TrainStep
    from stnf.models import STInterpMLP
    from stnf.utils import baselines as BL
    from stnf.utils import grid_scores
    d = T.dev()
    coords, z, masks = _field()
    torch.manual_seed(11)
    m = STInterpMLP(p=0, k_spatial_centers=[25, 81], k_temporal_centers=[10], hidden_dims=[64, 32], dropout=0.0).to(d)
    ti, si = np.nonzero(masks[0] & np.isfinite(z))
    eng = TrainStep(m.train(), lr=2e-2, max_batch=len(si), ema_decay=None)
    for _ in range(30):
        eng.step(None, torch.from_numpy(coords[si]).to(d), torch.from_numpy((ti / 6).astype(np.float32)).to(d),
                 torch.from_numpy(z[ti, si][:, None]).to(d))
    torch.cuda.synchronize()
    m.eval()
    config = {"baselines": True, "baseline_kriging": True, "kriging_levels": [0.05, 0.95]}
    plain = grid_scores(m, z, coords, *masks, config={"baselines": True})
    got = grid_scores(m, z, coords, *masks, config=config)
    assert set(got) == set(plain) and set(got["baseline"]) == set(plain["baseline"]) | {"kriging"}
    np.testing.assert_equal({k: a for k, a in got.items() if k != "baseline"},
                            {k: a for k, a in plain.items() if k != "baseline"})
    base = got["baseline"]
    np.testing.assert_equal({k: v for k, v in base.items() if k not in ("kriging", "skill", "site_skill")},
                            {k: v for k, v in plain["baseline"].items() if k not in ("skill", "site_skill")})
    alone = BL.grid_baselines(z, coords, *masks, config=config, device=d)
    np.testing.assert_equal(base["kriging"], alone["kriging"])
    assert list(base["skill"]) == ["nearest", "idw", "kriging"] and base["site_skill"].shape == (3, 150)
    assert np.array_equal(base["site_skill"][:2], plain["baseline"]["site_skill"], equal_nan=True)
    for s in ("all", "train", "valid", "test"):
        assert base["skill"]["kriging"][s] == 1.0 - got["splits"][s]["mse"] / base["kriging"]["splits"][s]["mse"]
        assert np.isfinite([base["kriging"]["splits"][s][n] for n in ("mse", "crps", "coverage")]).all()
    assert np.isfinite(base["site_skill"][2]).sum() == int(masks[2][0].sum())
    print("kriging:", base["kriging"]["variogram_fit"], base["kriging"]["msse"], "skill", base["skill"]["kriging"])
