"""The site-structured cases of tests/golden/site_cases.py, checked where no GPU is needed: that every batch keeps the
rows-per-cell condition, has the structure the GPU tests rely on (a crowded cell, knots nothing reaches, rows at
distance 0 from a knot, a second batch that reaches a strict subset of the first one's knots), that the float64
reference puts no more hidden units next to a ReLU kink than the GPU tests allow to flip, that an honest fp32
evaluation passes site_cases.compare_step at TOL with a margin -- and that a subtly wrong one does not."""
import numpy as np
import pytest

from golden import cases
from golden import site_cases as sc
from oracle import stdadk_oracle as orc
from oracle import torch_f64

_CACHE = {}


def _f64(model, sites):
    """(cfg, batch, float64 reference, near-kink alternatives) of a case of table (a), computed once."""
    if (model, sites) not in _CACHE:
        cfg, b = sc.module_case(model, sites)
        params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
        yo, lo, go, alts = orc.train_step_grads(b["X"], b["coords"], b["t"], b["y"], params, cfg, kink_tol=sc.KINK_TOL)
        _CACHE[(model, sites)] = (cfg, b, dict(y=yo, loss=lo, grads=go), alts)
    return _CACHE[(model, sites)]


def _f32(cfg, b):
    y, lo, g = orc.train_step_grads(b["X"], b["coords"], b["t"], b["y"], cases.make_state(cfg), cfg, dtype=np.float32)
    return dict(y=y, loss=lo, grads=g)


def _sequence_trajectory(name):
    """[(batch, float64 reference, alts)] of a sequence's three steps, each at the parameters the float64 optimiser
    (clip + AdamW of SEQ_OPT) leaves after the steps before it."""
    if name not in _CACHE:
        res, cfg, o = sc.resident(), sc.SEQ_CFG, sc.SEQ_OPT
        params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
        mm = {k: np.zeros_like(v) for k, v in params.items()}
        vv = {k: np.zeros_like(v) for k, v in params.items()}
        sh = {k: v.copy() for k, v in params.items()}
        out = []
        for i, idx in enumerate(sc.sequence_batches(name, res)):
            b = sc.take(res, idx)
            yo, lo, go, alts = torch_f64.train_step_grads(None, b["coords"], b["t"], b["y"], params, cfg, chunk=2048,
                                                          kink_tol=sc.KINK_TOL)
            out.append((b, {k: v.copy() for k, v in params.items()}, dict(y=yo, loss=lo, grads=go), alts))
            coef = orc.adamw_ema_step(params, go, mm, vv, sh, i + 1, o["lr"], o["weight_decay"], o["betas"], o["eps"],
                                      o["grad_clip"], o["ema_decay"])
            assert coef < 0.5                                   # clipping active
        _CACHE[name] = out
    return _CACHE[name]


# ------------------------------------------------------------------ site sets
def test_site_sets_are_what_they_say():
    bl = sc.blobs()
    assert bl.shape == (300, 2) and bl.dtype == np.float32 and bl[:, 0].max() <= np.float32(0.8)
    assert bl.min() >= 0.0 and bl[:, 1].max() <= 1.0
    for model in sc.MODELS:
        cfg = sc.model_cfg(model)
        cen, _, sides = orc.uniform_knots(cfg["k_spatial_centers"])
        ok = sc.site_set("on_knots", cfg)
        n = min(200, len(np.unique(cen, axis=0)))
        assert ok.shape == (n, 2) and ok.dtype == np.float32 and len(np.unique(ok, axis=0)) == n
        off = 0
        for side in sides:                                       # knots of every level, its corners among them
            lvl = {c.tobytes() for c in cen[off:off + side * side]}
            assert sum(s.tobytes() in lvl for s in ok) >= 12
            off += side * side
        have = {s.tobytes() for s in ok}
        for corner in ((0, 0), (0, 1), (1, 0), (1, 1)):
            assert np.array(corner, np.float32).tobytes() in have
        for axis, v in ((0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0)):  # points on each edge besides the corners
            assert (ok[:, axis] == v).sum() > 2
    bd = sc.border()
    assert bd.shape == (64, 2)
    on = np.isin(bd, np.array(sc.BORDER_VALUES, np.float32))
    assert on.any(1).all() and all((bd == np.float32(v)).any() for v in sc.BORDER_VALUES)
    oc = sc.one_cell()
    assert oc.shape == (6, 2) and len(np.unique(oc, axis=0)) == 6
    for G in (32, 64, 128, 256):
        k = orc.cell_keys(oc, G)
        assert len(set(k[:5])) == 1 and k[5] != k[0]
        u = oc[:5].astype(np.float64) * G                        # not on a cell edge
        assert (np.abs(u - np.round(u)) > 0.01).all()
    assert sc.single_site().shape == (1, 2)


def test_batches_repeat_coordinates_exactly():
    b = sc.batch(sc.blobs(), 1003, 1)
    assert len(np.unique(b["coords"], axis=0)) <= 300 and b["y"].shape == (1003, 1) and b["X"].shape == (1003, 0)
    assert np.array_equal(b["coords"], sc.blobs()[b["site"]])
    assert set(np.round(b["t"].ravel() * (sc.T_GRID - 1)).astype(int)) <= set(range(sc.T_GRID))
    b2 = sc.batch(sc.border(), 50, 2, p=3, Q=2)
    assert b2["X"].shape == (50, 3) and b2["y"].shape == (50, 2)
    mx = sc.mixed([b, sc.batch(sc.one_cell(), 200, 3)], 4)
    assert mx["coords"].shape == (1203, 2) and mx["y"].shape == (1203, 1)
    assert sorted(map(bytes, mx["coords"])) == sorted(map(bytes, np.concatenate([b["coords"], sc.batch(sc.one_cell(), 200, 3)["coords"]])))


# ------------------------------------------------------------------ the rows-per-cell condition
def test_no_batch_puts_more_than_2048_rows_into_one_cell():
    res = sc.resident()
    seen = []
    for model, sites in sc.MODULE_CASES:
        cfg, b = sc.module_case(model, sites)
        seen.append((f"{model}/{sites}", b["coords"], None, sites == "one_cell"))
    for name in sc.SEQUENCES:
        for i, idx in enumerate(sc.sequence_batches(name, res)):
            seen.append((f"{name}/batch{i + 1}", res["coords"][idx], None, i > 0))
    for B, G in sc.BIN_CASES:
        seen.append((f"bin{B}", sc.bin_batch(B)["coords"], G, True))
    for label, coords, G, crowded in seen:
        B = len(coords)
        G = sc.pick_cell_grid(B) if G is None else G
        n = sc.rows_per_cell(coords, G)
        print(f"{label}: B {B} G {G} rows per cell <= {n}")
        assert n <= sc.MAX_ROWS_PER_CELL, label
        if crowded:
            # 1 000 rows in one cell wherever the batch is large enough to hold them; the 1 003-, 700- and 257-row
            # one_cell batches of table (a) put their five sites' share (5/6 of the rows) there
            assert n >= (1000 if B > 1200 else 0.8 * B), (label, n)
    assert sc.pick_cell_grid(4096) == 64 and sc.pick_cell_grid(8192) == 128 and sc.pick_cell_grid(8193) == 128
    assert sc.pick_cell_grid(1) == 8 and sc.pick_cell_grid(1003) == 32 and sc.pick_cell_grid(10 ** 6) == 256


# ------------------------------------------------------------------ table (a): structure, near-kink units, fp32 margin
@pytest.mark.parametrize("model,sites", sc.MODULE_CASES)
def test_module_case_structure_and_fp32_margin(model, sites):
    cfg, b, ref, alts = _f64(model, sites)
    dW0 = ref["grads"]["mlp.0.weight"]
    unreached = int((~sc.reached(dW0)).sum())
    assert len(alts) <= sc.NEAR_KINK[(model, sites)], len(alts)
    assert sc.max_flipped(model, sites) <= min(sc.NEAR_KINK[(model, sites)], 2)
    if sites == "on_knots":
        cen = orc.uniform_knots(cfg["k_spatial_centers"])[0]
        d = np.sqrt(((b["coords"][:, None, :] - cen[None, :, :]) ** 2).sum(-1, dtype=np.float32))
        assert d.dtype == np.float32 and ((d == 0).sum(1) >= 1).all()
    if sites == "blobs" and model.startswith("c2"):
        off = cfg["p"]
        for k in cfg["k_spatial_centers"]:
            side = int(np.sqrt(k))
            if side in (64, 72):
                assert np.all(dW0[:, off + (7 * side // 8) * side:off + k] == 0.0)
            off += k
    r = sc.compare_step(_f32(cfg, b), ref, alts, sc.TOL, sc.max_flipped(model, sites))
    print(f"{model}/{sites}: B {cfg['B']} rows per cell {sc.rows_per_cell(b['coords'])}; {len(alts)} near-kink units; "
          f"{unreached} unreached columns; fp32 oracle against float64: loss {r['loss']:.1e} y {r['y']:.1e} worst "
          f"gradient rel-L2 {r['worst']:.2e} ({r['worst_key']})")
    assert r["worst"] <= sc.TOL / 10                             # the margin the bound was kept for


@pytest.mark.parametrize("model,sites", [("c2_b257", "blobs"), ("default227", "one_cell"), ("four_levels", "border")])
def test_compare_step_has_teeth(model, sites):
    """The fp32 run that passes fails with one repeated row dropped, one site moved by 1e-4, or the dW0 column of one
    unreached knot at 1e-8."""
    cfg, b, ref, alts = _f64(model, sites)
    cap = sc.max_flipped(model, sites)
    good = _f32(cfg, b)
    sc.compare_step(good, ref, alts, sc.TOL, cap)
    # a row whose (site, time) pair occurs once more is lost; its prediction is put back so that y alone passes
    coords = b["coords"]
    j = next(i for i in range(len(coords)) if (coords[:i] == coords[i]).all(1).any())
    keep = np.arange(len(coords)) != j
    bad = _f32(dict(cfg, B=cfg["B"] - 1), {k: b[k][keep] for k in ("X", "coords", "t", "y")})
    bad["y"] = np.insert(bad["y"], j, ref["y"][j], axis=0)
    with pytest.raises(AssertionError):
        sc.compare_step(bad, ref, alts, sc.TOL, cap)
    # one site 1e-4 away from where it is
    moved = dict(b, coords=b["coords"].copy())
    rows = (moved["coords"] == moved["coords"][j]).all(1)
    moved["coords"][rows, 0] += np.float32(1e-4)
    with pytest.raises(AssertionError):
        sc.compare_step(_f32(cfg, moved), ref, alts, sc.TOL, cap)
    # a stale row of dW0^T: far below any rel-L2 bound, caught by the exact-zero check only
    col = np.nonzero(~sc.reached(ref["grads"]["mlp.0.weight"]))[0][0]
    stale = dict(good, grads={k: v.copy() for k, v in good["grads"].items()})
    stale["grads"]["mlp.0.weight"][3, col] = 1e-8
    with pytest.raises(AssertionError, match="unreached"):
        sc.compare_step(stale, ref, alts, sc.TOL, cap)


def test_kink_fit_handles_repeated_rows():
    """A near-kink unit of a (site, time) pair that occurs k times is k identical columns of the least-squares fit;
    an fp32 run takes all k from the same side.  The minimum-norm solution gives each copy the coefficient 1."""
    rs = np.random.RandomState(0)
    g = {"a": rs.standard_normal((4, 3)), "b": rs.standard_normal(3)}
    d = {"a": 1e-3 * rs.standard_normal((4, 3)), "b": 1e-3 * rs.standard_normal(3)}
    e = {"a": 1e-3 * rs.standard_normal((4, 3)), "b": 1e-3 * rs.standard_normal(3)}
    alts = [((0, 5, 7), d), ((0, 9, 7), {k: v.copy() for k, v in d.items()}), ((1, 2, 3), e)]
    got = {k: g[k] + 2 * d[k] for k in g}
    flipped, adj = orc.fit_kink_sides(got, g, alts)
    assert sorted(flipped) == [(0, 5, 7), (0, 9, 7)]
    assert all(np.allclose(adj[k], got[k], rtol=0, atol=1e-15) for k in g)


# ------------------------------------------------------------------ sequences
@pytest.mark.parametrize("name", list(sc.SEQUENCES))
def test_sequence_reaches_a_strict_subset_after_the_first_batch(name):
    steps = _sequence_trajectory(name)
    first = sc.reached(steps[0][2]["grads"]["mlp.0.weight"])
    for i, (b, params, ref, alts) in enumerate(steps):
        now = sc.reached(ref["grads"]["mlp.0.weight"])
        print(f"{name} step {i + 1}: rows per cell {sc.rows_per_cell(b['coords'])}; {len(alts)} near-kink units; "
              f"{int(now.sum())} columns reached, {int((~now).sum())} unreached")
        assert len(alts) <= sc.SEQ_MAX_FLIPPED[name][i] <= 2
        if i > 0:
            assert not (now & ~first).any() and (first & ~now).sum() > 1000


def test_sequence_fp32_oracle_passes():
    """The 4 096-row sequence, each step at the float32 rounding of its float64 parameters (measured: worst gradient
    rel-L2 1.1e-6, 9 times under TOL; the 1 003-row cases of table (a) stay under TOL / 10)."""
    for i, (b, params, ref, alts) in enumerate(_sequence_trajectory("seq4096")):
        p32 = {k: v.astype(np.float32) for k, v in params.items()}
        p64 = {k: v.astype(np.float64) for k, v in p32.items()}
        yo, lo, go, alts = torch_f64.train_step_grads(None, b["coords"], b["t"], b["y"], p64, sc.SEQ_CFG, chunk=2048,
                                                      kink_tol=sc.KINK_TOL)
        y, l32, g = orc.train_step_grads(b["X"], b["coords"], b["t"], b["y"], p32, sc.SEQ_CFG, dtype=np.float32)
        r = sc.compare_step(dict(y=y, loss=l32, grads=g), dict(y=yo, loss=lo, grads=go), alts, sc.TOL, len(alts))
        print(f"seq4096 step {i + 1}: fp32 oracle against float64: loss {r['loss']:.1e} y {r['y']:.1e} worst gradient "
              f"rel-L2 {r['worst']:.2e} ({r['worst_key']}), flipped {r['flipped']}")


# ------------------------------------------------------------------ the chunked torch reference on a site case
@pytest.mark.parametrize("model,sites", [("c2_b257", "one_cell"), ("four_levels", "blobs")])
def test_torch_f64_equals_numpy_oracle_on_site_case(model, sites):
    cfg, b, ref, alts = _f64(model, sites)
    params = {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}
    yo, lo, go, alts_t = torch_f64.train_step_grads(b["X"], b["coords"], b["t"], b["y"], params, cfg, chunk=300,
                                                    kink_tol=sc.KINK_TOL)
    assert np.abs(yo - ref["y"]).max() <= 1e-12 and abs(lo - ref["loss"]) <= 1e-12 * ref["loss"]
    for k in go:
        assert sc.rel_l2(go[k], ref["grads"][k]) <= 1e-12, k
    assert np.array_equal(sc.reached(go["mlp.0.weight"]), sc.reached(ref["grads"]["mlp.0.weight"]))
    assert sorted(u for u, _ in alts_t) == sorted(u for u, _ in alts)
