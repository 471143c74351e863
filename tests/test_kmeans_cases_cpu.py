"""The CPU half of the balanced k-means initialiser's tests (tests/test_gpu_kmeans_balanced.py), no GPU needed:
  * the float64 restatement (golden/kmeans_cases.py) reaches the cost of the scipy.optimize.linear_sum_assignment oracle
    on every case, and regenerating a committed fit fixture reproduces it;
  * the comparator, at the GPU tests' own bound B, refuses a cost-raising swap, a nearest-then-greedy-repair assignment
    and a count one outside [lo, hi], and those wrong answers' cost gaps are at least 1000 B;
  * the constants kmeans_cases names are the kernels'; the header, the exports and stnf._native agree;
  * stnf.knot_init's host-side pieces equal the restatement's, and random_site's knots are what they were before the
    bandwidth helper was shared;
  * the argument checks of the new entry points, in a child process under STDADK_DRY_RUN=1 (validates, launches
    nothing)."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden import kmeans_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in kc.CASES]


@functools.lru_cache(maxsize=None)
def solved(name):
    """(inputs, costs, the oracle's optimum and labels, the restatement's iteration) of a case, computed once."""
    case = next(c for c in kc.CASES if c["name"] == name)
    inp = kc.case_inputs(case)
    c = kc.costs(inp["X"], inp["mu"])
    optimum, labels = kc.oracle(c, inp["lo"], inp["hi"])
    stats = {}
    res = kc.iteration(inp["X"], inp["mu"], inp["lo"], inp["hi"], stats)
    return inp, c, optimum, labels, dict(res, augmentations=stats["augmentations"])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reaches_the_oracles_cost(name):
    inp, c, optimum, labels, res = solved(name)
    kc.compare_assignment(labels, c, inp["lo"], inp["hi"], optimum, name + " (oracle)")
    kc.compare_assignment(res["labels"], c, inp["lo"], inp["hi"], optimum, name)
    assert res["inertia"] == kc.assignment_cost(c, res["labels"])
    k = c.shape[1]
    assert np.array_equal(res["mu"], kc.m_step(inp["X"], res["labels"], k)) and res["shift"] >= 0.0


def test_the_case_table_holds_what_the_issue_lists():
    by = {c["name"]: c for c in kc.CASES}
    assert any(c["n"] % c["k"] == 0 and 1 < c["k"] < c["n"] for c in kc.CASES)
    assert any(c["k"] == 1 for c in kc.CASES) and any(c["k"] == c["n"] > 1 for c in kc.CASES)
    assert any(c["family"] == "sites" and c["n"] > 2 * kc.N_SITES for c in kc.CASES)
    assert any(c["family"] == "identical" for c in kc.CASES)
    # both bounds binding: in the optimum one cluster sits on lo and another on hi, lo < hi
    inp, c, _, labels, _ = solved("clustered_n97_k9")
    cnt = np.bincount(labels, minlength=9)
    assert inp["lo"] < inp["hi"] and cnt.min() == inp["lo"] and cnt.max() == inp["hi"]
    # a centre no point is nearest to
    for name in ("clustered_n130_k25_far", "uniform_n61_k7_far"):
        inp, c, _, labels, _ = solved(name)
        assert (c.argmin(axis=1) != by[name]["k"] - 1).all() and (labels == by[name]["k"] - 1).sum() == inp["lo"]
    # n % k == 0: exactly n / k each
    inp, c, _, labels, res = solved("clustered_n60_k6")
    assert (np.bincount(res["labels"], minlength=6) == 10).all()
    for e in (kc.KM_T, kc.KM_AT):
        assert {e - 1, e, e + 1} <= {c["n"] for c in kc.CASES}
    assert {kc.KM_KT - 1, kc.KM_KT, kc.KM_KT + 1, kc.KM_MAX_K} <= {c["k"] for c in kc.CASES}


# ---- the comparator has teeth -----------------------------------------------------------------------------------------
def _degenerate(c):
    """Cases on which every feasible assignment costs the same: one cluster, or every cost equal."""
    return c.shape[1] == 1 or float(c.max()) == float(c.min())


@pytest.mark.parametrize("name", NAMES)
def test_comparator_refuses_a_cost_raising_swap(name):
    inp, c, optimum, labels, _ = solved(name)
    bad = kc.worst_swap(c, labels)
    if _degenerate(c):
        assert bad is None                      # nothing can raise the cost: there is no such wrong answer
        return
    assert bad is not None
    B = kc.bound_B(*c.shape, float(c.max()))
    assert kc.assignment_cost(c, bad) - optimum >= 1000.0 * B, (name, kc.assignment_cost(c, bad) - optimum, B)
    with pytest.raises(AssertionError, match="cost gap"):
        kc.compare_assignment(bad, c, inp["lo"], inp["hi"], optimum, name)


@pytest.mark.parametrize("name", NAMES)
def test_comparator_refuses_greedy_repair(name):
    """Nearest centre, then greedy repair: feasible on every case, optimal only where the nearest assignment needs no
    or almost no repair; wherever it is not optimal the comparator refuses it, and by at least 1000 B."""
    inp, c, optimum, _, _ = solved(name)
    bad = kc.greedy_repair(c, inp["lo"], inp["hi"])
    cnt = np.bincount(bad, minlength=c.shape[1])
    assert cnt.min() >= inp["lo"] and cnt.max() <= inp["hi"]
    gap = kc.assignment_cost(c, bad) - optimum
    B = kc.bound_B(*c.shape, float(c.max()))
    if gap <= B:
        kc.compare_assignment(bad, c, inp["lo"], inp["hi"], optimum, name)
        return
    assert gap >= 1000.0 * B, (name, gap, B)
    with pytest.raises(AssertionError, match="cost gap"):
        kc.compare_assignment(bad, c, inp["lo"], inp["hi"], optimum, name)


def test_greedy_repair_is_wrong_where_the_repair_is_real():
    """The cases whose nearest-centre assignment needs ten or more unit moves: greedy is off by more than 1000 B on
    every one of them (so an E-step that repaired greedily could not pass the GPU test)."""
    hard = 0
    for name in NAMES:
        inp, c, optimum, _, res = solved(name)
        if res["augmentations"] < 10 or _degenerate(c):
            continue
        hard += 1
        gap = kc.assignment_cost(c, kc.greedy_repair(c, inp["lo"], inp["hi"])) - optimum
        assert gap >= 1000.0 * kc.bound_B(*c.shape, float(c.max())), (name, gap)
    assert hard >= 15


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("which", ["lo", "hi"])
def test_comparator_refuses_a_count_one_outside_the_bounds(name, which):
    inp, c, optimum, labels, _ = solved(name)
    bad = kc.break_bound(c, labels, inp["lo"], inp["hi"], which)
    cnt = np.bincount(labels, minlength=c.shape[1])
    if bad is None:                             # one cluster, or no cluster of the optimum sits on that bound
        assert c.shape[1] == 1 or not (cnt == inp[which]).any()
        return
    with pytest.raises(AssertionError, match="counts"):
        kc.compare_assignment(bad, c, inp["lo"], inp["hi"], optimum, name)


def test_every_bound_is_broken_somewhere():
    for which in ("lo", "hi"):
        n_broken = sum(kc.break_bound(s[1], s[3], s[0]["lo"], s[0]["hi"], which) is not None for s in map(solved, NAMES))
        assert n_broken >= 15, (which, n_broken)


# ---- fits, constants, host-side pieces --------------------------------------------------------------------------------
def test_regenerating_a_fit_fixture_reproduces_it():
    from golden import make_kmeans_golden as mg
    case = kc.FIT_CASES[0]
    fx = np.load(os.path.join(kc.HERE, f"kmeans_{case['name']}.npz"))
    X = kc.fit_points(case)
    assert np.array_equal(fx["X"], X) and np.array_equal(fx["seeds"], mg.seeds_of(X, case["k"]))
    res = kc.fit(X, case["k"], list(fx["seeds"]))
    assert res["n_iter"] == fx["n_iter"].tolist() and res["best"] == int(fx["best"])
    assert np.array_equal(res["centers"], fx["centers"]) and res["inertias"] == fx["inertias"].tolist()
    for r, h in enumerate(res["history"]):
        assert (np.diff(h) <= 0.0).all() and np.array_equal(fx["history"][r, :len(h)], h)


@pytest.mark.parametrize("name", [c["name"] for c in kc.FIT_CASES])
def test_fit_fixtures_are_complete(name):
    case = next(c for c in kc.FIT_CASES if c["name"] == name)
    fx = np.load(os.path.join(kc.HERE, f"kmeans_{name}.npz"))
    assert fx["X"].shape == (kc.FIT_N, 2) and fx["seeds"].shape == (3, case["k"]) and fx["seeds"].max() < kc.FIT_N
    assert fx["centers"].shape == (case["k"], 2) and fx["n_iter"].max() < kc.MAX_ITER
    assert float(fx["inertias"].min()) == float(fx["inertias"][int(fx["best"])])


def test_named_constants_are_the_kernels():
    assert kc.kernel_constants() == dict(KM_T=kc.KM_T, KM_KT=kc.KM_KT, KM_AT=kc.KM_AT, KM_MAX_K=kc.KM_MAX_K)
    from stnf import _native as N
    assert N.KMEANS_MAX_K == kc.KM_MAX_K
    for n, k in ((1, 1), (10000, 121), (1023, 1023), (257, 7)):
        ints = k * k + k * n + n
        assert N.kmeans_workspace_bytes(n, k) == 8 * (n * k + k * k + -(-n // kc.KM_T) + 1) + 4 * (ints + ints % 2), (n, k)


def test_header_exports_and_native_agree():
    from stnf import _native as N
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stdadk.h")).read(), flags=re.S)
    new = {"stdadk_kmeans_workspace_bytes", "stdadk_kmeans_balanced_iter_f64"}
    assert new <= set(re.findall(r"\b(stdadk_[a-z0-9_]+)\s*\(", hdr)) and new <= set(N.exported_symbols())
    proto = re.search(r"int stdadk_kmeans_balanced_iter_f64\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(proto.split(",")) == len(N._SIGNATURES["stdadk_kmeans_balanced_iter_f64"][1]) == 13
    assert int(re.search(r"#define\s+STDADK_ABI_VERSION\s+(\d+)", hdr).group(1)) == N.ABI_VERSION == 10
    for sym in new:
        assert hasattr(N.lib(), sym)
    assert "kmeans" in open(os.path.join(ROOT, "st-dadk_amd", "csrc", "build.sh")).read()


def test_host_side_pieces_of_knot_init_equal_the_restatement():
    from stnf import knot_init
    for n, k in ((1, 1), (10, 10), (60, 6), (97, 9), (10000, 25), (10000, 81), (10000, 121)):
        assert knot_init.balanced_bounds(n, k) == kc.bounds(n, k)
        lo, hi = kc.bounds(n, k)
        assert 1 <= lo <= hi and k * lo <= n <= k * hi
    with pytest.raises(ValueError):
        knot_init.balanced_bounds(5, 6)
    c = kc.points("clustered", 25, 4)
    for k, k0 in ((25, 25), (3, 25), (2, 25), (1, 25), (1, 1)):
        bw = knot_init.neighbour_bandwidths(c[:k], k, k0)
        assert np.array_equal(torch.from_numpy(bw).float().numpy(), kc.knots32(c[:k], k, k0)[1])


def test_random_site_knots_are_unchanged_by_the_shared_helper():
    """_init_random_site as it was written before the helper was shared, restated here, against the module: bit for bit
    (its committed goldens pin the same through tests/test_host_cpu.py and the GPU parity tests)."""
    from scipy.spatial.distance import cdist
    from golden import cases
    from stnf.models.st_interp import SpatialBasisEmbedding
    pts = cases.init_points()
    for n_centers in ([25, 81], [1, 9], [4], [1]):
        np.random.seed(11)
        emb = SpatialBasisEmbedding(n_centers=n_centers, init_method='random_site', train_coords=pts)
        np.random.seed(11)
        cs, bs = [], []
        for k in n_centers:
            c = pts[np.random.choice(len(pts), k, replace=k > len(pts))]
            dist = cdist(c, c)
            np.fill_diagonal(dist, np.inf)
            nn = min(4, k - 1) if k > 1 else 1
            bw = 2.5 * np.sort(dist, axis=1)[:, :nn].mean(axis=1)
            if k == 1:
                side = int(np.sqrt(n_centers[0]))
                bw = np.array([2.5 * (1.0 / (side - 1) if side > 1 else 1.0)])
            cs.append(torch.from_numpy(c).float())
            bs.append(torch.from_numpy(bw).float())
        assert torch.equal(emb.centers, torch.cat(cs)) and torch.equal(emb.bandwidths, torch.cat(bs))


def test_init_device_plumbing_without_a_gpu():
    from stnf.models import create_model
    from stnf.models.st_interp import SpatialBasisEmbedding
    coords = kc.points("uniform", 64, 3).astype(np.float32)
    with pytest.raises(NotImplementedError, match="k_means_constrained"):            # the host path is as it was
        SpatialBasisEmbedding(n_centers=[4], init_method='kmeans_balanced', train_coords=coords)
    with pytest.raises(RuntimeError, match="HIP device"):
        SpatialBasisEmbedding(n_centers=[4], init_method='kmeans_balanced', train_coords=coords, init_device='cpu')
    with pytest.raises(RuntimeError, match="HIP device"):
        create_model(dict(k_spatial_centers=[4], k_temporal_centers=[5], hidden_dims=[16],
                          spatial_init_method='kmeans_balanced', spatial_init_device='cpu'), train_coords=coords)


# ---- the entries' argument checks ---------------------------------------------------------------------------------
def drive():
    """Child process under STDADK_DRY_RUN=1: messages of the entries' argument checks."""
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    import ctypes as C
    from stnf import _native as N
    n, k = 1000, 121
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)                      # noqa: E731
    rec = {"need": N.kmeans_workspace_bytes(n, k)}

    def call(key, n=n, k=k, lo=None, hi=None, short=0, alias=None, null=None):
        blo, bhi = kc.bounds(n, k) if 1 <= k <= n else (1, max(n, 1))
        lo, hi = blo if lo is None else lo, bhi if hi is None else hi
        a = dict(X=z(n, 2), mu=z(k, 2), mu_out=z(k, 2), labels=z(n, dt=torch.int32), stats=z(2), status=z(2, dt=torch.int32))
        ws = z(max(N.lib().stdadk_kmeans_workspace_bytes(max(n, 1), min(max(k, 1), 1023)) // 8 - short, 1))
        if alias == "mu":
            a["mu_out"] = a["mu"]
        if alias == "ws":
            a["mu_out"] = ws[:2 * k].view(k, 2)
        try:
            if null is not None:
                ptr = {name: t.data_ptr() for name, t in a.items()}
                ptr[null] = None
                rc = N.lib().stdadk_kmeans_balanced_iter_f64(
                    ptr["X"], n, k, ptr["mu"], lo, hi, ptr["mu_out"], ptr["labels"], ptr["stats"], ptr["status"],
                    ws.data_ptr(), ws.numel() * 8, None)
                N._check(rc, "stdadk_kmeans_balanced_iter_f64")
            else:
                N.kmeans_balanced_iter(a["X"], a["mu"], lo, hi, a["mu_out"], a["labels"], a["stats"], a["status"], ws)
            rec[key] = None
        except RuntimeError as e:
            rec[key] = str(e)
    call("good")
    call("good_small", n=1, k=1)
    call("good_k_eq_n", n=50, k=50)
    for name in ("X", "mu", "mu_out", "labels", "stats", "status"):
        call("null_" + name, null=name)
    call("k_gt_n", n=100, k=101, lo=1, hi=1)
    call("lo_k_gt_n", lo=9)                  # 9 x 121 = 1089 > 1000
    call("hi_k_lt_n", lo=7, hi=8)            # 8 x 121 = 968 < 1000
    call("lo_gt_hi", lo=8, hi=7)
    call("lo0", lo=0)
    call("n0", n=0, k=1, lo=1, hi=1)
    call("k0", k=0, lo=1, hi=1)
    call("k_big", n=2000, k=1024)
    call("alias_mu", alias="mu")
    call("alias_ws", alias="ws")
    call("workspace", short=1)
    for key, args in (("ws_n0", (0, 5)), ("ws_k0", (5, 0)), ("ws_k_big", (5000, 1024)), ("ws_nk_big", (1 << 22, 512))):
        try:
            N.kmeans_workspace_bytes(*args)
            rec[key] = None
        except RuntimeError as e:
            rec[key] = str(e)
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
    assert rec["good"] is None and rec["good_small"] is None and rec["good_k_eq_n"] is None and rec["profiled"] is None
    assert rec["launches"] == ["km_max_kernel", "km_scale_kernel", "km_q_kernel", "km_nearest_kernel", "km_balance_kernel",
                               "km_mean_kernel", "km_finish_kernel"]


@pytest.mark.parametrize("case,word", [
    ("null_X", "NULL"), ("null_mu", "NULL"), ("null_mu_out", "NULL"), ("null_labels", "NULL"), ("null_stats", "NULL"),
    ("null_status", "NULL"), ("k_gt_n", "k=101 clusters on n=100"), ("lo_k_gt_n", "exceeds n"), ("hi_k_lt_n", "below n"),
    ("lo_gt_hi", "lo <= hi"), ("lo0", "lo <= hi"), ("n0", "n=0"), ("k0", "k=0"), ("k_big", "k=1024"),
    ("alias_mu", "alias"), ("alias_ws", "alias"), ("workspace", "workspace"), ("ws_n0", "bad sizes"),
    ("ws_k0", "bad sizes"), ("ws_k_big", "bad sizes"), ("ws_nk_big", "bad sizes")])
def test_entry_refuses_bad_arguments(rec, case, word):
    assert rec[case] is not None and word in rec[case], rec[case]


@pytest.mark.parametrize("case,code", [("null_X", -1), ("k_gt_n", -2), ("lo_k_gt_n", -2), ("hi_k_lt_n", -2),
                                       ("workspace", -4)])
def test_entry_error_codes(rec, case, code):
    assert f"(code {code})" in rec[case], rec[case]


if __name__ == "__main__":
    drive()
