"""The cell-binned neighbour search on the device: stdadk_knn_cells_f32 through the ABI on every case of
tests/golden/knn_cells_cases.py, on pre-filled outputs and a pre-filled workspace -- nbr_idx equal and nbr_d2 bit-equal
to knn_host AND to stdadk_knn_f32's own output -- determinism (against the order its atomics give inside a cell too),
empty sides, every error code of the brute-force search's table with everything writable left untouched, a captured
graph; then grid_baselines and rasterize_nearest with the search switched, bit for bit against the brute-force result."""
import numpy as np
import pytest
import torch

from golden import knn_cases as kc
from golden import knn_cells_cases as cc
import test_gpu_knn as K
import test_gpu_parity as T

pytestmark = pytest.mark.gpu


def search_cells(case, fill=-7):
    """One call on pre-filled outputs and a pre-filled workspace; returns the device tensors (nbr_idx, nbr_d2)."""
    from stnf import _native as N
    d = T.dev()
    M, S, k = len(case["q"]), len(case["coords"]), case["k"]
    nM = 1 if case["src"] is None else len(case["src"])
    idx = torch.full((nM, M, k), fill, dtype=torch.int32, device=d)
    d2 = torch.full((nM, M, k), float(fill), dtype=torch.float64, device=d)
    ws = torch.full((N.knn_cells_workspace_bytes(M, S, nM, k) // 8,), float(fill), dtype=torch.float64, device=d)
    N.knn_cells(K._to(d, case["q"]), K._to(d, case["coords"]), K._to(d, case["src"]), k, case["exclude_self"], idx, d2, ws)
    return idx, d2


@pytest.fixture(scope="module")
def host_tables():
    """(case, knn_host's table) of every case: computed once, never changed."""
    from stnf.utils import baselines as BL
    return [(c, BL.knn_host(c["q"], c["coords"], c["src"], c["k"], c["exclude_self"])) for c in cc.all_cases()]


def test_the_table_equals_knn_host_and_the_brute_force_search_on_every_case(host_tables):
    outs = [(search_cells(c), K.search(c)) for c, _ in host_tables]      # (the launches are all queued before the reads)
    sides = set()
    for (case, (want_idx, want_d2)), ((idx, d2), (b_idx, b_d2)) in zip(host_tables, outs):
        assert kc.same_table(idx.cpu().numpy(), d2.cpu().numpy(), want_idx, want_d2), case["name"]
        assert torch.equal(idx, b_idx) and torch.equal(d2.view(torch.int64), b_d2.view(torch.int64)), case["name"]
        sides.add(cc.grid_side(len(case["coords"])))
    print(f"{len(outs)} cases, grid sides {sorted(sides)}")
    assert sides >= set(range(1, 33))


def test_same_call_same_bits():
    case = kc.span_seam_case()
    a, b = search_cells(case, fill=-7), search_cells(case, fill=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int((a[0] >= 0).sum()) == a[0].numel()


def test_the_order_inside_a_cell_cannot_move_the_table():
    """Clusters: tens of sites per cell, scattered by atomics; targets of one cell in any order over the waves."""
    case = cc.cluster_case()
    counts = np.diff(cc.binning(case["q"], case["coords"])["start"])[:-1]
    assert counts.max() > 10 * cc.OCC
    first = search_cells(case)
    for fill in (1, 2, 3, 4, 5):
        again = search_cells(case, fill=fill)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1].view(torch.int64), again[1].view(torch.int64))


def test_empty_sides():
    """M = 0 or nM = 0 writes nothing; S = 0 (and a slice without sources) writes the neutral rows."""
    from stnf import _native as N
    base = kc.make_case(65, 40, 8, 1, seed=5)
    idx, d2 = search_cells(dict(base, q=base["q"][:0]))
    assert idx.shape == (1, 0, 8)
    idx, d2 = search_cells(dict(base, src=np.zeros((0, 40), dtype=np.uint8)))
    assert idx.shape == (0, 65, 8)
    idx, d2 = search_cells(dict(base, coords=base["coords"][:0]))
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all()) and idx.shape == (1, 65, 8)
    idx, d2 = search_cells(dict(base, src=np.zeros((2, 40), dtype=np.uint8)))
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all()) and idx.shape == (2, 65, 8)
    assert N.knn_cells_workspace_bytes(0, 0, 0, 1) > 0


def _raw(d, M=70, S=300, nM=1, k=8, exclude_self=0, src=False, idx_off=0, d2_off=0, ws_off=0, ws_short=0, q_off=0,
         alias=None, null=None):
    """test_gpu_knn._raw against the new entry and its workspace function: the C call with one thing wrong; returns
    (code, whether everything it could have written is untouched)."""
    from stnf import _native as N
    lib = N.lib()
    ok = lambda n: n if 0 < n < 2 ** 20 else 1                   # noqa: E731  (a refused size is never indexed)
    nq, ns, nm, kk = ok(M), ok(S), ok(nM), k if 0 < k <= 16 else 1
    q, coords = torch.zeros(nq + 1, 2, device=d), torch.zeros(ns, 2, device=d)
    flags = torch.ones(nm, ns, dtype=torch.uint8, device=d)
    need = lib.stdadk_knn_cells_workspace_bytes(M, S, nM, k)
    idx = torch.full((nm * nq * kk + 2,), 3, dtype=torch.int32, device=d)
    d2 = torch.full((nm * nq * kk + 2,), 3.0, dtype=torch.float64, device=d)
    ws = torch.full((need // 8 + 2,), 3.0, dtype=torch.float64, device=d)
    ptr = {"q": q.data_ptr() + q_off, "coords": coords.data_ptr(), "src": flags.data_ptr() if src or nM != 1 else None,
           "idx": idx.data_ptr() + idx_off, "d2": d2.data_ptr() + d2_off, "ws": ws.data_ptr() + ws_off}
    if alias:
        ptr[alias[0]] = ptr[alias[1]]
    if null:
        ptr[null] = None
    rc = lib.stdadk_knn_cells_f32(ptr["q"], M, ptr["coords"], S, ptr["src"], nM, k, exclude_self, ptr["idx"], ptr["d2"],
                                  ptr["ws"], max(need - ws_short, 0), None)
    torch.cuda.synchronize()
    return rc, bool((idx == 3).all()) and bool((d2 == 3.0).all()) and bool((ws == 3.0).all())


# the table of wrong arguments of test_gpu_knn.test_every_error_code_of_the_search, as it stands there
WRONG = next(m for m in K.test_every_error_code_of_the_search.pytestmark if m.name == "parametrize").args[1]


@pytest.mark.parametrize("what,kw,code", WRONG)
def test_every_error_code_of_the_search(what, kw, code):
    from stnf import _native as N
    lib = N.lib()
    sizes = lib.stdadk_knn_cells_workspace_bytes
    assert (sizes(-1, 5, 1, 1), sizes(5, 2 ** 31, 1, 1), sizes(5, 5, 1, 0), sizes(5, 5, 1, 17), sizes(2 ** 27, 5, 2, 8)) == (0,) * 5
    rc, untouched = _raw(T.dev(), **kw)
    assert rc == code and untouched, (what, rc, lib.stdadk_last_error())
    assert _raw(T.dev())[0] == 0 and _raw(T.dev(), M=300, exclude_self=1, src=True)[0] == 0      # the good calls succeed


def test_the_error_table_is_the_brute_force_searchs():
    assert len(WRONG) == 25 and {code for _, _, code in WRONG} == {-1, -2, -3, -4}


def test_a_captured_call_replays_the_direct_calls_bytes():
    """One graph with a single branch: the six launches of one call, in stream order."""
    from stnf import _native as N
    d = T.dev()
    case = kc.make_case(130, 300, 8, 3, "lattice", density=0.5, seed=41)
    q, c, src = (K._to(d, case[n]) for n in ("q", "coords", "src"))
    eager = search_cells(case)
    idx, d2 = torch.full_like(eager[0], -7), torch.full_like(eager[1], -7.0)
    ws = torch.empty(N.knn_cells_workspace_bytes(130, 300, 3, 8) // 8, dtype=torch.float64, device=d)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        N.knn_cells(q, c, src, 8, False, idx, d2, ws)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager[0]) and torch.equal(d2.view(torch.int64), eager[1].view(torch.int64))


@pytest.mark.parametrize("site_wise", [True, False])
@pytest.mark.parametrize("kriging", [False, True])
def test_grid_baselines_with_the_cells_search_equal_the_brute_force_result(site_wise, kriging):
    from stnf.utils import baselines as BL
    d = T.dev()
    coords, z, masks = K._field(site_wise=site_wise)
    config = {"baseline_k": 4}
    if kriging:
        config.update({"baseline_kriging": True, "kriging_model": "spherical", "kriging_params": (0.1, 1.0, 0.4),
                       "kriging_levels": [0.1, 0.9], "kriging_k": 8})
    for max_rows in (None, 3 * 150):
        brute = BL.grid_baselines(z, coords, *masks, config=config, max_rows=max_rows, device=d)
        named = BL.grid_baselines(z, coords, *masks, config=dict(config, baseline_search="brute"), max_rows=max_rows, device=d)
        cells = BL.grid_baselines(z, coords, *masks, config=dict(config, baseline_search="cells"), max_rows=max_rows, device=d)
        assert cells["shared_table"] == site_wise and set(cells) == set(brute) and ("kriging" in cells) == kriging
        np.testing.assert_equal(named, brute)
        np.testing.assert_equal(cells, brute)                    # every key, NaN positions included
    assert np.isfinite(cells["idw"]["splits"]["test"]["mse"]) and np.isfinite(cells["train_dist"]).all()
    with pytest.raises(ValueError, match="search"):
        BL.grid_baselines(z, coords, *masks, config={"baseline_search": "tree"}, device=d)


@pytest.mark.parametrize("n_sites,ny,nx", kc.RASTER_CASES)
def test_rasters_with_the_cells_search_are_the_brute_force_rasters(n_sites, ny, nx):
    from stnf.utils import baselines as BL
    case = kc.make_raster_case(n_sites, ny, nx)
    rows = np.stack([case["values"], np.where(np.arange(n_sites) % 3 == 0, np.nan, case["values"])]).astype(np.float32)
    for values in (case["values"], rows):
        brute = BL.rasterize_nearest(case["coords"], values, resolution=(ny, nx), device=T.dev())
        cells = BL.rasterize_nearest(case["coords"], values, resolution=(ny, nx), device=T.dev(), search="cells")
        assert all(kc.same_bits(a, b) for a, b in zip(cells, brute)) and np.isfinite(cells[0]).all()
    with pytest.raises(ValueError, match="search"):
        BL.rasterize_nearest(case["coords"], case["values"], resolution=(ny, nx), device=T.dev(), search="tree")
