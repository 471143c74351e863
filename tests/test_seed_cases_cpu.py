"""k-means++ seeding on the device, the parts that need no GPU.

  * The numpy restatement of the contract (golden/seed_cases.py) on the pre-drawn random stream gives the coordinates of
    every seed set that sklearn.cluster.kmeans_plusplus recorded (golden/seed_*.npz, gmm_fit_*.npz, kmeans_fit_*.npz; none
    left out): the stream is drawn in sklearn's order, and stnf.knot_init.kmeanspp_stream draws that stream.
  * The comparator has teeth: one altered uniform, and one swapped candidate, fail it.
  * No fixed case is decided by the rounding of a sum: numpy's sums and the kernel's summation order pick the same seeds
    on every edge case and every recorded case (golden/seed_cases.py RESEEDED lists the data seeds that were replaced).
  * SpatialBasisEmbedding / create_model refuse a bad init_seeding / spatial_init_seeding.
  * The argument checks of stdadk_kmeanspp_f64, in a child process under STDADK_DRY_RUN=1 (validates, launches nothing)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden import seed_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_NAMES = [c["name"] for c in sc.EDGE_CASES] + [c["name"] for c in sc.DEGENERATE_CASES]


# ---- the restatement against sklearn ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SKLEARN_CASES)
def test_restatement_reproduces_sklearn(name):
    fx = sc.sklearn_case(name)
    X, seeds = fx["X"], fx["seeds"]
    assert seeds.shape[0] == sc.N_INIT and fx["u"].shape == (sc.N_INIT, seeds.shape[1] - 1, sc.trials(seeds.shape[1]))
    rows, pots, _ = sc.restate_runs(X, seeds.shape[1], fx["first"], fx["u"])
    moved = sc.compare_seeds(X, rows, seeds, name)
    print(f"{name}: {moved} of {seeds.size} indices name another row of the same site; pots {pots}")
    assert np.array_equal(rows[:, 0], seeds[:, 0])                 # the first rows are drawn, not computed
    assert len(np.unique(X, axis=0)) > seeds.shape[1]              # k below the number of distinct points


def test_the_library_draws_the_same_stream():
    from stnf import knot_init
    assert knot_init.N_INIT == sc.N_INIT and knot_init.RANDOM_STATE == sc.RANDOM_STATE
    levels = [1, 2, 25, 81, 121]
    assert [knot_init.kmeanspp_trials(k) for k in (1, 2, 3, 7, 8, 20, 21, 54, 55, 148, 149, 403, 404, 1096, 1097)] == \
        [2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9]
    for k, (first, u) in zip(levels, knot_init.kmeanspp_stream(700, levels)):
        want_first, want_u = sc.draw_stream(700, k, sc.N_INIT)
        assert first.dtype == np.int32 and u.dtype == np.float64 and u.shape == (3, k - 1, sc.trials(k))
        assert np.array_equal(first, want_first) and np.array_equal(u, want_u)
        assert (u >= 0).all() and (u < 1).all()


def test_stream_against_the_installed_sklearn():
    """Live, not recorded: kmeanspp_seeds (sklearn on the host) against the restatement on kmeanspp_stream."""
    from stnf import knot_init
    X = sc.points("clustered", 700, 11)
    levels = [9, 25, 60]
    host = knot_init.kmeanspp_seeds(X, levels)
    for k, seeds, (first, u) in zip(levels, host, knot_init.kmeanspp_stream(len(X), levels)):
        rows, _, _ = sc.restate_runs(X, k, first, u)
        sc.compare_seeds(X, rows, np.stack(seeds), f"k={k}")


# ---- the comparator's teeth ---------------------------------------------------------------------------------------
def test_comparator_rejects_an_altered_uniform_and_a_swapped_candidate():
    fx = sc.sklearn_case("kmeans_fit_uniform_k25")
    X, seeds, k = fx["X"], fx["seeds"], 25
    rows, _, picks, _ = sc.restate(X, k, int(fx["first"][0]), fx["u"][0])
    sc.compare_seeds(X, rows[None], seeds[:1], "unaltered")
    # the uniform behind the chosen candidate of step 3, moved by half the range
    u = fx["u"][0].copy()
    u[2, picks[3]] = (u[2, picks[3]] + 0.5) % 1.0
    bad = sc.restate(X, k, int(fx["first"][0]), u)[0]
    assert np.array_equal(bad[:3], rows[:3])
    with pytest.raises(AssertionError, match="differ in coordinates"):
        sc.compare_seeds(X, bad[None], seeds[:1], "altered uniform")
    # the second-best candidate at step 5
    bad = sc.restate(X, k, int(fx["first"][0]), fx["u"][0],
                     choose=lambda c, pots: np.argsort(pots, kind="stable")[1 if c == 5 else 0])[0]
    assert np.array_equal(bad[:5], rows[:5])
    with pytest.raises(AssertionError, match="differ in coordinates"):
        sc.compare_seeds(X, bad[None], seeds[:1], "swapped candidate")
    # another row of the same site is the same seed; a row out of range is not
    dup = np.concatenate([X, X[rows[4]][None]])
    moved = rows.copy()
    moved[4] = len(X)
    assert sc.compare_seeds(dup, moved[None], rows[None], "same site") == 1
    with pytest.raises(AssertionError, match="out of range"):
        sc.compare_seeds(X, moved[None], rows[None], "out of range")


# ---- the fixed cases sit on no rounding boundary -------------------------------------------------------------------
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_no_edge_case_is_decided_by_rounding(name):
    """numpy's sums and the kernel's summation order pick the same seeds; the potentials differ by the order alone."""
    inp = sc.degenerate_inputs(name) if name.startswith("degenerate") else sc.edge_inputs(name)
    X, n = inp["X"], len(inp["X"])
    rows, pots, zero = sc.edge_expected(name)
    krows, kpots, kzero = sc.edge_expected(name, True)
    sc.compare_seeds(X, krows, rows, name)
    assert (np.abs(kpots - pots) <= sc.pot_bound(n, pots)).all() and np.array_equal(zero, kzero)
    assert inp["L"] == sc.trials(rows.shape[1]) <= sc.KPP_MAX_L
    if name.startswith("degenerate"):
        k = rows.shape[1]
        assert (zero == inp["distinct"]).all() and inp["distinct"] < k          # pot reaches 0 once every site is chosen
        for r in range(len(rows)):
            assert (rows[r, zero[r]:] == 0).all() and pots[r] == 0.0


def test_recorded_cases_are_not_decided_by_rounding():
    for name in sc.SKLEARN_CASES:
        fx = sc.sklearn_case(name)
        rows, _, _ = sc.restate_runs(fx["X"], fx["seeds"].shape[1], fx["first"], fx["u"],
                                     rows=sc.rows_per_thread(len(fx["X"])))
        sc.compare_seeds(fx["X"], rows, fx["seeds"], name)


def test_every_kernel_edge_is_in_the_case_table():
    src = open(os.path.join(ROOT, "st-dadk_amd", "csrc", "kmeanspp.hip")).read()
    const = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (KPP_[A-Z_]+) = (\d+);", src)}
    assert const["KPP_T"] == sc.KPP_T and const["KPP_MAX_R"] == sc.KPP_MAX_R == sc.KPP_ROWS[-1]
    assert const["KPP_MAX_L"] == sc.KPP_MAX_L and const["KPP_MAX_RUNS"] == sc.KPP_MAX_RUNS and const["KPP_MAX_K"] == sc.KPP_MAX_K
    assert tuple(int(r) for r in re.findall(r"KPP_GO\(RegRows<(\d+)>\)", src)) + (sc.KPP_MAX_R,) == sc.KPP_ROWS
    ns, ks, runs = ({c[key] for c in sc.EDGE_CASES} for key in ("n", "k", "runs"))
    assert {1, 2, 63, 64, 65, 1023, 1024, 1025, 10000} <= ns and max(ns) > sc.KPP_T * sc.KPP_MAX_R
    for r in sc.KPP_ROWS:
        assert {sc.KPP_T * r, sc.KPP_T * r + 1} <= ns, r
    assert {1, 2, 3, 8, 21, 55, 149, 404, 1097} <= ks and runs == {1, 3, sc.KPP_MAX_RUNS}
    assert any(c["n"] == c["k"] > 2 and c["family"] == "uniform" for c in sc.EDGE_CASES)
    assert [sc.rows_per_thread(n) for n in (1, 1024, 1025, 2049, 4097, 7169, 10240, 10241, 20000)] == [1, 1, 2, 4, 7, 10, 10, 11, 20]


# ---- constructor and config ----------------------------------------------------------------------------------------
def test_constructor_refuses_bad_seeding():
    from stnf.models import create_model
    from stnf.models.st_interp import SpatialBasisEmbedding, STInterpMLP
    pts = sc.points("uniform", 300, 3).astype(np.float32)
    for method in ("uniform", "gmm", "random_site", "kmeans_balanced"):
        with pytest.raises(ValueError, match="init_seeding"):
            SpatialBasisEmbedding(n_centers=[9], init_method=method, train_coords=pts, init_seeding="gpu")
    for method in ("gmm", "kmeans_balanced"):
        with pytest.raises(ValueError, match="init_device"):
            SpatialBasisEmbedding(n_centers=[9], init_method=method, train_coords=pts, init_seeding="device")
        with pytest.raises(ValueError, match="init_device"):
            create_model(dict(k_spatial_centers=[9], k_temporal_centers=[5], hidden_dims=[16], spatial_init_method=method,
                              spatial_init_seeding="device"), train_coords=pts)
    with pytest.raises(ValueError, match="init_seeding"):
        STInterpMLP(k_spatial_centers=[9], k_temporal_centers=[5], hidden_dims=[16], spatial_init_seeding="sklearn")
    # for uniform and random_site the key does nothing; the default is the host
    a = SpatialBasisEmbedding(n_centers=[9, 25])
    b = SpatialBasisEmbedding(n_centers=[9, 25], init_seeding="device")
    assert torch.equal(a.centers, b.centers) and torch.equal(a.bandwidths, b.bandwidths)
    np.random.seed(4)
    a = SpatialBasisEmbedding(n_centers=[9], init_method="random_site", train_coords=pts)
    np.random.seed(4)
    b = create_model(dict(k_spatial_centers=[9], k_temporal_centers=[5], hidden_dims=[16], spatial_init_method="random_site",
                          spatial_init_seeding="device"), train_coords=pts).spatial_basis
    assert torch.equal(a.centers, b.centers) and torch.equal(a.bandwidths, b.bandwidths)
    # the host gmm path is what it was, with the key absent or 'host'
    np.random.seed(4)
    a = SpatialBasisEmbedding(n_centers=[9], init_method="gmm", train_coords=pts)
    np.random.seed(4)
    b = SpatialBasisEmbedding(n_centers=[9], init_method="gmm", train_coords=pts, init_seeding="host")
    assert torch.equal(a.centers, b.centers) and torch.equal(a.bandwidths, b.bandwidths)


def test_knot_functions_refuse_bad_seeding():
    from stnf import knot_init
    pts = sc.points("uniform", 50, 3)
    for fn in (knot_init.gmm_knots, knot_init.balanced_kmeans_knots):
        with pytest.raises(ValueError, match="seeding"):
            fn(pts, [9], "cuda", seeding="gpu")


# ---- the entry's argument checks -----------------------------------------------------------------------------------
def drive():
    """Child process under STDADK_DRY_RUN=1: messages of the entry's argument checks."""
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    from stnf import _native as N
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)                      # noqa: E731
    rec = {}

    def call(key, n=1000, k=121, runs=3, L=6, short=0, alias=None, null=None, odd=None):
        a = dict(X=z(n, 2), first=z(max(runs, 1), dt=torch.int32), u=z(max(runs, 1), max(k - 1, 0), max(L, 1)),
                 idx_out=z(max(runs, 1), max(k, 1), dt=torch.int32), pot_out=z(max(runs, 1)))
        need = N.lib().stdadk_kmeanspp_workspace_bytes(n, k, runs) or 8
        ws = z(max(need // 8 - short, 1) + 1)
        if alias == "first":
            a["idx_out"] = a["first"].view(1, 1)
        if alias == "u":
            a["pot_out"] = a["u"].view(-1)[:runs]
        if alias == "ws":
            ws = a["pot_out"]
        ptr = {name: t.data_ptr() for name, t in a.items()}
        ptr["ws"], ws_bytes = ws.data_ptr(), (ws.numel() - 1) * 8
        if null is not None:
            ptr[null] = None
        if odd is not None:
            ptr[odd] += 4 if odd in ("X", "u", "pot_out", "ws") else 2
        rc = N.lib().stdadk_kmeanspp_f64(ptr["X"], n, k, runs, L, ptr["first"], ptr["u"], ptr["idx_out"], ptr["pot_out"],
                                         ptr["ws"], ws_bytes, None)
        try:
            N._check(rc, "stdadk_kmeanspp_f64")
            rec[key] = None
        except RuntimeError as e:
            rec[key] = str(e)

    call("good")
    call("good_n1", n=1, k=1, runs=1, L=2)
    call("good_k_eq_n", n=50, k=50, runs=64, L=16)
    call("good_memory_path", n=10241, k=8, runs=3, L=4)
    call("good_k1_null_u", k=1, null="u")
    for name in ("X", "first", "u", "idx_out", "pot_out", "ws"):
        call("null_" + name, null=name)
    for name in ("X", "first", "u", "idx_out", "pot_out", "ws"):
        call("odd_" + name, odd=name)
    call("n0", n=0, k=1)
    call("k0", k=0)
    call("k_gt_n", n=100, k=101)
    call("k_big", n=70000, k=65537)
    call("runs0", runs=0)
    call("runs_big", runs=65)
    call("L0", L=0)
    call("L_big", L=17)
    call("alias_first", n=5, k=1, runs=1, alias="first")
    call("alias_u", alias="u")
    call("alias_ws", alias="ws")
    call("workspace", n=10241, k=8, runs=3, L=4, short=1)
    rec["need_registers"] = N.kmeanspp_workspace_bytes(10240, 8, 3)
    rec["need_memory"] = N.kmeanspp_workspace_bytes(10241, 8, 3)
    for key, args in (("ws_n0", (0, 1, 1)), ("ws_k0", (5, 0, 1)), ("ws_k_gt_n", (5, 6, 1)), ("ws_runs0", (5, 5, 0)),
                      ("ws_runs_big", (5, 5, 65)), ("ws_n_big", (1 << 31, 5, 1))):
        try:
            N.kmeanspp_workspace_bytes(*args)
            rec[key] = None
        except RuntimeError as e:
            rec[key] = str(e)
    # the wrapper's own checks
    for key, kw in (("wrap_dtype", dict(first=z(3))), ("wrap_shape", dict(u=z(3, 119, 6))), ("wrap_X", dict(X=z(1000, 3)))):
        a = dict(X=z(1000, 2), first=z(3, dt=torch.int32), u=z(3, 120, 6), idx_out=z(3, 121, dt=torch.int32), pot_out=z(3),
                 workspace=z(1))
        a.update(kw)
        try:
            N.kmeanspp(**a)
            rec[key] = None
        except RuntimeError as e:
            rec[key] = str(e)
    N.kmeanspp(z(1000, 2), z(3, dt=torch.int32), z(3, 120, 6), z(3, 121, dt=torch.int32), z(3), z(1))
    N.profile_enable(True)
    call("profiled")
    rec["launches"] = [name for name, _ in N.profile_collect()]
    print("RECORD " + json.dumps(rec))


@pytest.fixture(scope="module")
def rec():
    env = dict(os.environ, STDADK_DRY_RUN="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RECORD ")][-1]
    return json.loads(line[len("RECORD "):])


def test_entry_accepts_good_arguments(rec):
    for key in ("good", "good_n1", "good_k_eq_n", "good_memory_path", "good_k1_null_u", "profiled"):
        assert rec[key] is None, (key, rec[key])
    assert rec["launches"] == ["kmeanspp_kernel"]
    assert rec["need_registers"] == 8 and rec["need_memory"] == 3 * 10241 * 8


@pytest.mark.parametrize("case,code,word", [
    ("null_X", -1, "NULL"), ("null_first", -1, "NULL"), ("null_u", -1, "NULL"), ("null_idx_out", -1, "NULL"),
    ("null_pot_out", -1, "NULL"), ("null_ws", -1, "NULL"), ("n0", -1, "n=0"), ("k0", -1, "k=0"), ("k_gt_n", -1, "k=101"),
    ("k_big", -1, "k=65537"), ("runs0", -1, "runs=0"), ("runs_big", -1, "runs=65"), ("L0", -1, "L=0"), ("L_big", -1, "L=17"),
    ("alias_first", -1, "alias"), ("alias_u", -1, "alias"), ("alias_ws", -1, "alias"),
    ("odd_X", -3, "aligned"), ("odd_first", -3, "aligned"), ("odd_u", -3, "aligned"), ("odd_idx_out", -3, "aligned"),
    ("odd_pot_out", -3, "aligned"), ("odd_ws", -3, "aligned"), ("workspace", -4, "workspace")])
def test_entry_refuses_bad_arguments(rec, case, code, word):
    assert rec[case] is not None and word in rec[case] and f"(code {code})" in rec[case], rec[case]


@pytest.mark.parametrize("case", ["ws_n0", "ws_k0", "ws_k_gt_n", "ws_runs0", "ws_runs_big", "ws_n_big"])
def test_workspace_refuses_bad_sizes(rec, case):
    assert rec[case] is not None and "bad sizes" in rec[case], rec[case]


@pytest.mark.parametrize("case,word", [("wrap_dtype", "first must be a contiguous torch.int32"),
                                       ("wrap_shape", "u must be a contiguous torch.float64 tensor of shape (3, 120, 6)"),
                                       ("wrap_X", "X must be (n, 2)")])
def test_wrapper_checks(rec, case, word):
    assert rec[case] is not None and word in rec[case], rec[case]


if __name__ == "__main__":
    drive()
