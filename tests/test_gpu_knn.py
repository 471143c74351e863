"""Neighbour tables on the device: stdadk_knn_f32 and stdadk_knn_apply_f32 through the ABI on every generated case of
tests/golden/knn_cases.py, on pre-filled outputs -- nbr_idx equal and nbr_d2 bit-equal to knn_host, nearest and idw
bit-equal to knn_apply_host at every power, NaN positions included -- determinism, empty sides, every error code with
everything writable left untouched, a captured graph; then grid_baselines and rasterize_nearest on the device against
the host route, and grid_scores' `baseline` entry on a small trained model."""
import numpy as np
import pytest
import torch

from golden import knn_cases as kc
import test_gpu_parity as T

pytestmark = pytest.mark.gpu


def _to(d, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(d)


def search(case, fill=-7):
    """One call on pre-filled outputs (both are ASSIGNED); returns the device tensors (nbr_idx, nbr_d2)."""
    from stnf import _native as N
    d = T.dev()
    M, S, k = len(case["q"]), len(case["coords"]), case["k"]
    nM = 1 if case["src"] is None else len(case["src"])
    idx = torch.full((nM, M, k), fill, dtype=torch.int32, device=d)
    d2 = torch.full((nM, M, k), float(fill), dtype=torch.float64, device=d)
    ws = torch.full((N.knn_workspace_bytes(M, S, nM, k) // 8,), float(fill), dtype=torch.float64, device=d)
    N.knn(_to(d, case["q"]), _to(d, case["coords"]), _to(d, case["src"]), k, case["exclude_self"], idx, d2, ws)
    return idx, d2


def apply(idx, d2, k, z, power, fill=-7.0):
    from stnf import _native as N
    nT, M = z.shape[0], idx.shape[1]
    near = torch.full((nT, M), fill, dtype=torch.float32, device=z.device)
    idw = torch.full((nT, M), fill, dtype=torch.float32, device=z.device)
    N.knn_apply(idx, d2, k, z, power, near, idw)
    return near, idw


@pytest.fixture(scope="module")
def host_tables():
    """(case, knn_host's table) of every generated case: computed once, never changed."""
    from stnf.utils import baselines as BL
    return [(c, BL.knn_host(c["q"], c["coords"], c["src"], c["k"], c["exclude_self"])) for c in kc.all_cases()]


def test_search_and_apply_equal_the_host_statements_on_every_case(host_tables):
    from stnf.utils import baselines as BL
    d = T.dev()
    outs = [search(c) for c, _ in host_tables]                   # (the launches are all queued before the reads)
    spans, values = set(), 0
    for (case, (want_idx, want_d2)), (idx, d2) in zip(host_tables, outs):
        what = (case["q"].shape, case["coords"].shape, case["k"], case["exclude_self"])
        assert kc.same_table(idx.cpu().numpy(), d2.cpu().numpy(), want_idx, want_d2), what
        spans.add(kc.spans(len(case["q"]), len(case["coords"]), idx.shape[0])[0])
        z = _to(d, case["z"])
        for power in kc.POWERS:
            for k in {case["k"], max(1, case["k"] // 2)}:
                near, idw = (a.cpu().numpy() for a in apply(idx, d2, k, z, power))
                want_near, want = BL.knn_apply_host(want_idx, want_d2, k, case["z"], power)
                assert kc.same_bits(near, want_near) and kc.same_bits(idw, want), what + (power, k)
                values += int(np.isfinite(want).sum())
    print(f"{len(outs)} cases, span counts {sorted(spans)}, {values} finite idw values compared bit for bit")
    assert {0, 1, 2, 5} <= spans and values > 10000


def test_same_call_same_bits_and_one_output_at_a_time():
    from stnf import _native as N
    case = kc.span_seam_case()
    a, b = search(case, fill=-7), search(case, fill=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int((a[0] >= 0).sum()) == a[0].numel()
    z = _to(T.dev(), case["z"])
    near, idw = apply(*a, case["k"], z, 2)
    only = torch.full_like(idw, -7.0)
    N.knn_apply(*a, case["k"], z, 2, None, only)
    assert torch.equal(only.view(torch.int32), idw.view(torch.int32))
    N.knn_apply(*a, case["k"], z, 2, only, None)
    assert torch.equal(only.view(torch.int32), near.view(torch.int32))


def test_empty_sides():
    """M = 0 or nM = 0 writes nothing; S = 0 (and a slice without sources) writes the neutral rows; nT = 0 is no call."""
    from stnf import _native as N
    d = T.dev()
    base = kc.make_case(65, 40, 8, 1, seed=5)
    idx, d2 = search(dict(base, q=base["q"][:0]))
    assert idx.shape == (1, 0, 8)
    idx, d2 = search(dict(base, src=np.zeros((0, 40), dtype=np.uint8)))
    assert idx.shape == (0, 65, 8)
    idx, d2 = search(dict(base, coords=base["coords"][:0]))
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all()) and idx.shape == (1, 65, 8)
    near, idw = apply(idx, d2, 8, torch.zeros(3, 0, device=d), 2)
    assert bool(torch.isnan(near).all()) and bool(torch.isnan(idw).all())
    near, idw = apply(idx, d2, 8, torch.zeros(0, 0, device=d), 2)
    assert near.shape == (0, 65)
    idx, d2 = search(dict(base, src=np.zeros((2, 40), dtype=np.uint8)))
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all()) and idx.shape == (2, 65, 8)
    assert N.knn_workspace_bytes(0, 0, 0, 1) > 0


def _raw(d, M=70, S=300, nM=1, k=8, exclude_self=0, src=False, idx_off=0, d2_off=0, ws_off=0, ws_short=0, q_off=0,
         alias=None, null=None):
    """The C search itself with one thing wrong; returns (code, whether everything it could have written is untouched)."""
    from stnf import _native as N
    lib = N.lib()
    ok = lambda n: n if 0 < n < 2 ** 20 else 1                   # noqa: E731  (a refused size is never indexed)
    nq, ns, nm, kk = ok(M), ok(S), ok(nM), k if 0 < k <= 16 else 1
    q, coords = torch.zeros(nq + 1, 2, device=d), torch.zeros(ns, 2, device=d)
    flags = torch.ones(nm, ns, dtype=torch.uint8, device=d)
    need = lib.stdadk_knn_workspace_bytes(M, S, nM, k)
    idx = torch.full((nm * nq * kk + 2,), 3, dtype=torch.int32, device=d)
    d2 = torch.full((nm * nq * kk + 2,), 3.0, dtype=torch.float64, device=d)
    ws = torch.full((need // 8 + 2,), 3.0, dtype=torch.float64, device=d)
    ptr = {"q": q.data_ptr() + q_off, "coords": coords.data_ptr(), "src": flags.data_ptr() if src or nM != 1 else None,
           "idx": idx.data_ptr() + idx_off, "d2": d2.data_ptr() + d2_off, "ws": ws.data_ptr() + ws_off}
    if alias:
        ptr[alias[0]] = ptr[alias[1]]
    if null:
        ptr[null] = None
    rc = lib.stdadk_knn_f32(ptr["q"], M, ptr["coords"], S, ptr["src"], nM, k, exclude_self, ptr["idx"], ptr["d2"],
                            ptr["ws"], max(need - ws_short, 0), None)
    torch.cuda.synchronize()
    return rc, bool((idx == 3).all()) and bool((d2 == 3.0).all()) and bool((ws == 3.0).all())


@pytest.mark.parametrize("what,kw,code", [
    ("M < 0", dict(M=-1), -1), ("S = 2^31", dict(S=2 ** 31), -1), ("nM < 0", dict(nM=-1, src=True), -1),
    ("k = 0", dict(k=0), -1), ("k = 17", dict(k=17), -1), ("exclude_self with M != S", dict(exclude_self=1), -1),
    ("exclude_self = 2", dict(exclude_self=2, M=300), -1), ("src NULL with nM = 2", dict(nM=2, null="src"), -1),
    ("nM*M*k = 2^31", dict(M=2 ** 27, nM=2, k=8, src=True), -2), ("nM*M = 2^31", dict(M=2 ** 16, nM=2 ** 15, k=1, src=True), -2),
    ("NULL q", dict(null="q"), -1), ("NULL coords", dict(null="coords"), -1), ("NULL nbr_idx", dict(null="idx"), -1),
    ("NULL nbr_d2", dict(null="d2"), -1), ("NULL workspace", dict(null="ws"), -1),
    ("nbr_d2 aliases q", dict(alias=("d2", "q")), -1), ("nbr_idx aliases coords", dict(alias=("idx", "coords")), -1),
    ("nbr_idx aliases src", dict(src=True, alias=("idx", "src")), -1), ("nbr_idx aliases nbr_d2", dict(alias=("idx", "d2")), -1),
    ("nbr_d2 aliases the workspace", dict(alias=("d2", "ws")), -1),
    ("nbr_d2 misaligned", dict(d2_off=4), -3), ("nbr_idx misaligned", dict(idx_off=2), -3), ("q misaligned", dict(q_off=2), -3),
    ("workspace misaligned", dict(ws_off=4), -3), ("workspace short", dict(ws_short=8), -4)])
def test_every_error_code_of_the_search(what, kw, code):
    from stnf import _native as N
    lib = N.lib()
    sizes = lib.stdadk_knn_workspace_bytes
    assert (sizes(-1, 5, 1, 1), sizes(5, 2 ** 31, 1, 1), sizes(5, 5, 1, 0), sizes(5, 5, 1, 17), sizes(2 ** 27, 5, 2, 8)) == (0,) * 5
    rc, untouched = _raw(T.dev(), **kw)
    assert rc == code and untouched, (what, rc, lib.stdadk_last_error())
    assert _raw(T.dev())[0] == 0 and _raw(T.dev(), M=300, exclude_self=1, src=True)[0] == 0      # the good calls succeed


def _raw_apply(d, nM=1, M=70, k_tab=8, k=8, nT=3, S=300, power=2, idx_off=0, d2_off=0, near_off=0, idw_off=0, z_off=0,
               alias=None, null=()):
    from stnf import _native as N
    lib = N.lib()
    ok = lambda n: n if 0 < n < 2 ** 20 else 1                   # noqa: E731
    nm, nq, nt, ns, kk = ok(nM), ok(M), ok(nT), ok(S), k_tab if 0 < k_tab <= 16 else 1
    idx = torch.zeros(nm * nq * kk + 2, dtype=torch.int32, device=d)
    d2 = torch.ones(nm * nq * kk + 2, dtype=torch.float64, device=d)
    z = torch.zeros(nt * ns + 2, device=d)
    near, idw = torch.full((nt * nq + 2,), 3.0, device=d), torch.full((nt * nq + 2,), 3.0, device=d)
    ptr = {"idx": idx.data_ptr() + idx_off, "d2": d2.data_ptr() + d2_off, "z": z.data_ptr() + z_off,
           "near": near.data_ptr() + near_off, "idw": idw.data_ptr() + idw_off}
    if alias:
        ptr[alias[0]] = ptr[alias[1]]
    for name in null:
        ptr[name] = None
    rc = lib.stdadk_knn_apply_f32(ptr["idx"], ptr["d2"], nM, M, k_tab, k, ptr["z"], nT, S, power, ptr["near"], ptr["idw"],
                                  None)
    torch.cuda.synchronize()
    return rc, bool((near == 3.0).all()) and bool((idw == 3.0).all())


@pytest.mark.parametrize("what,kw,code", [
    ("M < 0", dict(M=-1), -1), ("S = 2^31", dict(S=2 ** 31), -1), ("nT < 0", dict(nT=-1), -1),
    ("nM neither 1 nor nT", dict(nM=2), -1), ("k = 0", dict(k=0), -1), ("k > k_tab", dict(k_tab=4, k=5), -1),
    ("k_tab = 17", dict(k_tab=17, k=1), -1), ("power 5", dict(power=5), -1), ("power < 0", dict(power=-1), -1),
    ("both outputs NULL", dict(null=("near", "idw")), -1), ("NULL table", dict(null=("idx",)), -1),
    ("NULL z", dict(null=("z",)), -1), ("nT*M = 2^31", dict(nT=2 ** 16, M=2 ** 15, S=1), -2),
    ("nT*S = 2^31", dict(nT=2 ** 16, M=1, S=2 ** 15), -2),
    ("idw aliases z", dict(alias=("idw", "z")), -1), ("nearest aliases nbr_d2", dict(alias=("near", "d2")), -1),
    ("nearest aliases idw", dict(alias=("near", "idw")), -1),
    ("nbr_d2 misaligned", dict(d2_off=4), -3), ("nbr_idx misaligned", dict(idx_off=2), -3), ("z misaligned", dict(z_off=2), -3),
    ("nearest misaligned", dict(near_off=2), -3), ("idw misaligned", dict(idw_off=2), -3)])
def test_every_error_code_of_the_apply(what, kw, code):
    from stnf import _native as N
    rc, untouched = _raw_apply(T.dev(), **kw)
    assert rc == code and untouched, (what, rc, N.lib().stdadk_last_error())
    assert _raw_apply(T.dev())[0] == 0 and _raw_apply(T.dev(), nM=3)[0] == 0                     # the good calls succeed


def test_wrapper_refuses_what_the_neighbouring_wrappers_refuse():
    from stnf import _native as N
    d = T.dev()
    q, c = torch.zeros(5, 2, device=d), torch.zeros(9, 2, device=d)
    idx, d2 = torch.zeros(1, 5, 2, dtype=torch.int32, device=d), torch.zeros(1, 5, 2, dtype=torch.float64, device=d)
    ws = torch.zeros(N.knn_workspace_bytes(5, 9, 1, 2) // 8, dtype=torch.float64, device=d)
    N.knn(q, c, None, 2, False, idx, d2, ws)
    for bad in (dict(q=q.double()), dict(q=q.cpu()), dict(idx=idx.long()), dict(d2=d2.float()), dict(d2=d2[:, :4]),
                dict(src=torch.ones(1, 8, dtype=torch.uint8, device=d)), dict(c=torch.zeros(9, 3, device=d))):
        a = dict(dict(q=q, c=c, src=None, idx=idx, d2=d2), **bad)
        with pytest.raises(RuntimeError):
            N.knn(a["q"], a["c"], a["src"], 2, False, a["idx"], a["d2"], ws)
    with pytest.raises(RuntimeError):
        N.knn_workspace_bytes(5, 9, 1, 17)
    z, out = torch.zeros(3, 9, device=d), torch.zeros(3, 5, device=d)
    N.knn_apply(idx, d2, 2, z, 2, out, None)
    for bad in (dict(z=z.double()), dict(out=out[:2]), dict(k=3), dict(power=7)):
        a = dict(dict(z=z, out=out, k=2, power=2), **bad)
        with pytest.raises(RuntimeError):
            N.knn_apply(idx, d2, a["k"], a["z"], a["power"], a["out"], None)


def test_a_captured_call_replays_the_direct_calls_bytes():
    from stnf import _native as N
    d = T.dev()
    case = kc.make_case(130, 300, 8, 3, "lattice", density=0.5, seed=41)
    q, c, src, z = (_to(d, case[n]) for n in ("q", "coords", "src", "z"))
    eager = search(case)
    eager_out = apply(*eager, 8, z, 2)
    idx, d2 = torch.full_like(eager[0], -7), torch.full_like(eager[1], -7.0)
    near, idw = torch.full_like(eager_out[0], -7.0), torch.full_like(eager_out[1], -7.0)
    ws = torch.empty(N.knn_workspace_bytes(130, 300, 3, 8) // 8, dtype=torch.float64, device=d)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        N.knn(q, c, src, 8, False, idx, d2, ws)
        N.knn_apply(idx, d2, 8, z, 2, near, idw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager[0]) and torch.equal(d2.view(torch.int64), eager[1].view(torch.int64))
    assert torch.equal(near.view(torch.int32), eager_out[0].view(torch.int32))
    assert torch.equal(idw.view(torch.int32), eager_out[1].view(torch.int32))


def _field(T_=7, S=150, seed=4, site_wise=True):
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = (np.sin(5 * coords[:, 0])[None, :] + rs.standard_normal((T_, S)) * 0.2).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.05] = np.nan
    code = np.broadcast_to(rs.randint(1, 4, size=S), (T_, S)) if site_wise else rs.randint(0, 4, size=(T_, S))
    if site_wise:
        z[:, code[0] == 1] = np.where(np.isnan(z[:, code[0] == 1]), 0.5, z[:, code[0] == 1])      # training sites complete
    return coords, z, [code == c for c in (1, 2, 3)]


def _close(got, ref, what):
    """grid_baselines' dicts, device against host.  The tables are exact, so both routes score the SAME float32
    predictions; the sums differ by their order only, within the 1e-12 relative test_gpu_grid_score.py holds
    stdadk_grid_score_f32 to, and a metric is one more rounded operation (a ratio, a square root) on top: 2^-52."""
    tol = 1e-12 + 2.0 ** -52
    for b in ("nearest", "idw"):
        for s, metrics in ref[b]["splits"].items():
            for name, v in metrics.items():
                g = got[b]["splits"][s][name]
                assert (np.isnan(v) and np.isnan(g)) or abs(g - v) <= tol * abs(v), (what, b, s, name, g, v)
            assert got[b]["splits"][s]["rows"] == metrics["rows"]
        for name in ("site_mse", "site_mse_by_split", "time_mse"):
            g, v = got[b][name], ref[b][name]
            assert np.array_equal(np.isnan(g), np.isnan(v)) and np.all(np.abs(g - v)[~np.isnan(v)] <= tol * np.abs(v)[~np.isnan(v)]), \
                (what, b, name)
    assert np.array_equal(got["train_dist"], ref["train_dist"])
    assert (got["k"], got["power"], got["shared_table"]) == (ref["k"], ref["power"], ref["shared_table"])


@pytest.mark.parametrize("site_wise", [True, False])
def test_grid_baselines_on_the_device_equal_the_host_route(site_wise):
    from stnf.utils import baselines as BL
    d = T.dev()
    coords, z, masks = _field(site_wise=site_wise)
    for config, max_rows in (({}, None), ({"baseline_k": 3, "baseline_power": 1}, 3 * 150)):
        host = BL.grid_baselines(z, coords, *masks, config=config, max_rows=max_rows)
        got = BL.grid_baselines(z, coords, *masks, config=config, max_rows=max_rows, device=d)
        assert got["shared_table"] == site_wise
        _close(got, host, (site_wise, config))
    assert np.isfinite(got["idw"]["splits"]["test"]["mse"]) and got["idw"]["splits"]["test"]["rows"] > 0


@pytest.mark.parametrize("n_sites,ny,nx", kc.RASTER_CASES)
def test_rasters_on_the_device_are_the_host_routes(n_sites, ny, nx):
    from stnf.utils import baselines as BL
    case = kc.make_raster_case(n_sites, ny, nx)
    rows = np.stack([case["values"], np.where(np.arange(n_sites) % 3 == 0, np.nan, case["values"])]).astype(np.float32)
    for values in (case["values"], rows):
        host = BL.rasterize_nearest(case["coords"], values, resolution=(ny, nx))
        got = BL.rasterize_nearest(case["coords"], values, resolution=(ny, nx), device=T.dev())
        assert all(kc.same_bits(a, b) for a, b in zip(got, host)) and np.isfinite(got[0]).all()


def test_grid_scores_baseline_entry_on_a_trained_model():
    """`baseline`, `skill` and `site_skill` present and consistent with the parts; the other entries bit-identical to a
    call without the key."""
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
    plain = grid_scores(m, z, coords, *masks)
    got = grid_scores(m, z, coords, *masks, config={"baselines": True})
    assert "baseline" not in plain and set(got) == set(plain) | {"baseline"}
    np.testing.assert_equal({k: a for k, a in got.items() if k != "baseline"}, plain)
    base = got["baseline"]
    alone = BL.grid_baselines(z, coords, *masks, device=d)
    np.testing.assert_equal({k: v for k, v in base.items() if k not in ("skill", "site_skill")}, alone)
    _close(alone, BL.grid_baselines(z, coords, *masks), "trained")
    assert base["shared_table"] and base["k"] == 8 and base["power"] == 2 and base["site_skill"].shape == (2, 150)
    for r, b in enumerate(("nearest", "idw")):
        for s in ("all", "train", "valid", "test"):
            assert base["skill"][b][s] == 1.0 - plain["splits"][s]["mse"] / base[b]["splits"][s]["mse"]
        with np.errstate(invalid="ignore", divide="ignore"):
            want = 1.0 - plain["site_mse_by_split"][3] / base[b]["site_mse_by_split"][3]
        assert np.array_equal(base["site_skill"][r], want, equal_nan=True)
        assert np.isfinite(base["site_skill"][r]).sum() == int(masks[2][0].sum())
    print("skill of the small trained model:", base["skill"])
