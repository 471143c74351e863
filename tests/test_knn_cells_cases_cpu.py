"""The cell-binned neighbour search, the half that runs anywhere: the python restatement of its plan
(tests/golden/knn_cells_cases.py) equals knn_host bit for bit on every case and does NOT when its stop is `>=`; the cases
cover what they must; the header, the exports, stnf._native and build.sh agree; the grid-rule constants are the unit's;
under the library's dry run (a child process: STDADK_DRY_RUN is read at import) a `cells` call lists its own launches
and a `brute` call what it always listed, and the entry refuses what stdadk_knn_f32 refuses; grid_baselines and
rasterize_nearest refuse an unknown search and the host route ignores the key."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden import knn_cases as kc
from golden import knn_cells_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the cases on which a search that stops on `bound >= worst` returns a wrong table: an equal distance at a lower index,
# in a ring not yet met, belongs in the row
STOP_ON_EQUAL_IS_WRONG_ON = {"knn_cases[17]", "knn_cases[18]", "knn_cases[26]", "lattice_edges", "S144_M130_k2_lattice_nM3"}


@pytest.fixture(scope="module")
def tables():
    """(case, knn_host's table) of every case: computed once, never changed."""
    from stnf.utils import baselines as BL
    return [(c, BL.knn_host(c["q"], c["coords"], c["src"], c["k"], c["exclude_self"])) for c in cc.all_cases()]


def _brute_pairs(case):
    return len(case["q"]) * (len(case["coords"]) if case["src"] is None else int((case["src"] != 0).sum()))


def test_the_restatement_equals_knn_host_on_every_case(tables):
    met = brute = 0
    for case, want in tables:
        idx, d2, pairs = cc.restate_cells(case)
        assert kc.same_table(idx, d2, *want), case["name"]
        assert pairs <= _brute_pairs(case), case["name"]
        met, brute = met + pairs, brute + _brute_pairs(case)
    print(f"{len(tables)} cases: {met} of {brute} pairs met")
    assert met < brute


def test_stopping_on_an_equal_bound_is_caught(tables):
    wrong = {case["name"] for case, want in tables if not kc.same_table(*cc.restate_cells(case, strict=False)[:2], *want)}
    print("`>=` is wrong on:", sorted(wrong))
    assert wrong >= STOP_ON_EQUAL_IS_WRONG_ON
    assert any(n.startswith("knn_cases[") for n in wrong) and "lattice_edges" in wrong


def test_cases_cover_what_they_must():
    cases = cc.all_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) and len([n for n in names if n.startswith("knn_cases[")]) == len(kc.all_cases())
    new = [c for c in cases if not c["name"].startswith("knn_cases[")]
    sizes = {len(c["coords"]) for c in new}
    changes = cc.rule_changes()
    assert changes[0] == 4 * cc.OCC and changes[-1] == 4096 and len(changes) == 31
    for s in changes:                                            # just below and at every change of the grid side
        assert {s - 1, s} <= sizes and cc.grid_side(s - 1) + 1 == cc.grid_side(s)
    assert {1, 2, 4097} <= sizes and cc.grid_side(1) == cc.grid_side(15) == 1 and cc.grid_side(4097) == 32
    assert cc.grid_side(2 ** 31 - 1) == cc.GMAX and cc.grid_side(0) == 1
    assert {len(c["q"]) for c in new} >= set(cc.SIZES_M) and {c["k"] for c in new} == set(kc.SIZES_K)
    by = {c["name"]: c for c in cases}
    fin = lambda a: a[np.isfinite(a).all(axis=1)]                # noqa: E731
    extent = lambda c: np.ptp(fin(c["coords"]), axis=0)          # noqa: E731
    assert (extent(by["coincident"]) == 0).all() and sorted(extent(by["one_line"]) == 0) == [False, True]
    # the lattice: every site on a cell edge, targets at cell corners and centres
    lat = by["lattice_edges"]
    b = cc.binning(lat["q"], lat["coords"])
    assert b["G"] == 4 and b["box"] == (0.0, 0.0, 4.0, 4.0) and (lat["coords"] * 4 == np.round(lat["coords"] * 4)).all()
    assert ((lat["q"] * 4) % 1 == 0).all(axis=1).sum() >= 25 and ((lat["q"] * 4) % 1 == 0.5).all(axis=1).sum() == 16
    # clusters: most cells empty, a few crowded
    b = cc.binning(by["clusters"]["q"], by["clusters"]["coords"])
    counts = np.diff(b["start"])[:-1]
    assert (counts == 0).mean() > 0.6 and counts.max() > 10 * cc.OCC
    # targets outside the box, near and far; non-finite targets and sources; only loose sites
    out = by["outside"]
    lo, hi = out["coords"].min(axis=0), out["coords"].max(axis=0)
    outside = ((out["q"] < lo) | (out["q"] > hi)).any(axis=1)
    assert outside.sum() > 20 and (np.abs(out["q"]) >= 1e6).any(axis=1).sum() == 8 and (np.abs(out["q"][outside]) < 2).all(axis=1).sum() > 10
    bad = by["non_finite"]
    for a in (bad["q"], bad["coords"]):
        assert np.isnan(a).any() and (a == np.inf).any() and (a == -np.inf).any()
    assert not np.isfinite(by["only_loose_sites"]["coords"]).any()
    # per-slice densities: 0.5, 0.02 (fewer than k within reach), fewer than k in total, none
    n_src = (by["densities"]["src"] != 0).sum(axis=1)
    assert 400 < n_src[0] < 600 and by["densities"]["k"] < n_src[1] < 40 and 0 < n_src[2] < by["densities"]["k"] and n_src[3] == 0
    dense = cc.restate_cells(dict(by["densities"], src=by["densities"]["src"][:1]))[2]
    sparse = cc.restate_cells(dict(by["densities"], src=by["densities"]["src"][1:2]))[2]
    print(f"pairs met: {dense} of {130 * n_src[0]} at density 0.5, {sparse} of {130 * n_src[1]} at 0.02")
    assert dense < 130 * n_src[0] and sparse / (130 * n_src[1]) > dense / (130 * n_src[0])      # more rings when sparse
    # leave-one-out with duplicated sites: the twin at d2 = 0 stays, self does not
    tw = by["twins_all"]
    idx, d2, _ = cc.restate_cells(tw)
    assert tw["exclude_self"] and (idx[0, :60, 0] == np.arange(100, 160)).all() and (d2[0, :60, 0] == 0).all()
    assert (idx[0, :, 0] != np.arange(160)).all() and by["twins"]["exclude_self"] and by["twins"]["src"] is not None
    # targets in an order that is not cell order
    for c in new:
        if len(c["q"]) > 1 and len(c["coords"]) >= 4 * cc.OCC and c["name"] not in ("coincident", "only_loose_sites"):
            cells = cc.binning(c["q"], c["coords"])["t_cell"]
            assert (np.diff(cells) < 0).any(), c["name"]


def test_the_header_the_exports_and_the_build_name_the_entry():
    from stnf import _native as N
    hdr = open(os.path.join(ROOT, "include", "stdadk.h")).read()
    new = {"stdadk_knn_cells_workspace_bytes", "stdadk_knn_cells_f32"}
    assert new <= set(re.findall(r"\b(stdadk_[a-z0-9_]+)\s*\(", hdr)) and new <= set(N.exported_symbols()) and new <= N._OWN_UNIT
    assert re.search(r"#define STDADK_ABI_VERSION (\d+)", hdr).group(1) == "10" and N.ABI_VERSION == 10
    assert "knn_cells" in open(os.path.join(ROOT, "st-dadk_amd", "csrc", "build.sh")).read().split()
    # one parameter list: the prototype of the new entry is that of stdadk_knn_f32, and so is the signature
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1))      # noqa: E731
    assert proto("stdadk_knn_cells_f32") == proto("stdadk_knn_f32")
    assert N._SIGNATURES["stdadk_knn_cells_f32"] == N._SIGNATURES["stdadk_knn_f32"]
    assert N._SIGNATURES["stdadk_knn_cells_workspace_bytes"] == N._SIGNATURES["stdadk_knn_workspace_bytes"]


def test_grid_rule_constants_are_the_units():
    src = open(os.path.join(ROOT, "st-dadk_amd", "csrc", "knn_cells.hip")).read()
    val = {"kWave": 64}
    for name, expr in re.findall(r"constexpr int (KC_\w+) = ([\w\s*/+-]+);", src):
        val[name] = int(eval(expr, {}, val))
    assert (val["KC_OCC"], val["KC_GMAX"], val["KC_MT"]) == (cc.OCC, cc.GMAX, cc.WAVE)
    assert "fp contract(off)" in src and "knn_insert<KT, true>" in src and "__ballot" in src
    knn = open(os.path.join(ROOT, "st-dadk_amd", "csrc", "knn.hip")).read()
    assert not re.findall(r"constexpr int KC_", knn) and not re.findall(r"constexpr int KN_", src)


# ---- the entry under the library's dry run ----------------------------------------------------------------------

WRONG = [("M < 0", dict(M=-1), -1), ("S = 2^31", dict(S=2 ** 31), -1), ("nM < 0", dict(nM=-1, src=True), -1),
         ("k = 0", dict(k=0), -1), ("k = 17", dict(k=17), -1), ("exclude_self with M != S", dict(exclude_self=1), -1),
         ("exclude_self = 2", dict(exclude_self=2, M=300), -1), ("src NULL with nM = 2", dict(nM=2, null="src"), -1),
         ("nM*M*k = 2^31", dict(M=2 ** 27, nM=2, k=8, src=True), -2), ("NULL q", dict(null="q"), -1),
         ("NULL workspace", dict(null="ws"), -1), ("nbr_d2 aliases q", dict(alias=("d2", "q")), -1),
         ("nbr_d2 aliases the workspace", dict(alias=("d2", "ws")), -1), ("nbr_d2 misaligned", dict(d2_off=4), -3),
         ("workspace misaligned", dict(ws_off=4), -3), ("workspace short", dict(ws_short=8), -4)]


def drive():
    """Child process under STDADK_DRY_RUN=1: the launches of a call by each search, and the codes of wrong calls."""
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    from stnf import _native as N
    from stnf.utils import baselines as BL
    lib = N.lib()
    rec = {"sizes": [lib.stdadk_knn_cells_workspace_bytes(*a) for a in
                     ((-1, 5, 1, 1), (5, 2 ** 31, 1, 1), (5, 5, 1, 0), (5, 5, 1, 17), (2 ** 27, 5, 2, 8), (0, 0, 0, 1), (70, 300, 1, 8))]}

    def raw(M=70, S=300, nM=1, k=8, exclude_self=0, src=False, d2_off=0, ws_off=0, ws_short=0, alias=None, null=None):
        ok = lambda n: n if 0 < n < 2 ** 20 else 1               # noqa: E731
        nq, ns, nm, kk = ok(M), ok(S), ok(nM), k if 0 < k <= 16 else 1
        need = lib.stdadk_knn_cells_workspace_bytes(M, S, nM, k)
        bufs = dict(q=torch.zeros(nq + 1, 2), coords=torch.zeros(ns, 2), src=torch.ones(nm, ns, dtype=torch.uint8),
                    idx=torch.zeros(nm * nq * kk + 2, dtype=torch.int32), d2=torch.zeros(nm * nq * kk + 2, dtype=torch.float64),
                    ws=torch.zeros(need // 8 + 2, dtype=torch.float64))
        ptr = {n: t.data_ptr() for n, t in bufs.items()}
        ptr["d2"] += d2_off
        ptr["ws"] += ws_off
        if not (src or nM != 1):
            ptr["src"] = None
        if alias:
            ptr[alias[0]] = ptr[alias[1]]
        if null:
            ptr[null] = None
        return lib.stdadk_knn_cells_f32(ptr["q"], M, ptr["coords"], S, ptr["src"], nM, k, exclude_self, ptr["idx"],
                                        ptr["d2"], ptr["ws"], max(need - ws_short, 0), None)
    rec["codes"] = [raw(**kw) for _, kw, _ in WRONG]
    rec["good"] = [raw(), raw(M=300, exclude_self=1, src=True), raw(S=0), raw(M=0)]
    q, c = torch.zeros(70, 2), torch.zeros(300, 2)
    for search in BL.SEARCHES:
        for S, k in ((300, 8), (0, 3)):
            N.profile_enable(True)                               # (since this call: the list starts again)
            BL.device_knn(q, c[:S], None, k, False, search)
            rec[f"{search}_S{S}"] = [name for name, ms in N.profile_collect() if ms == 0.0]
    print("RECORD " + json.dumps(rec))


@pytest.fixture(scope="module")
def rec():
    env = dict(os.environ, STDADK_DRY_RUN="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RECORD ")][-1]
    return json.loads(line[len("RECORD "):])


def test_each_search_lists_its_own_launches(rec):
    build = ["knn_cells_init_kernel", "knn_cells_bounds_kernel", "knn_cells_count_kernel", "knn_cells_scan_kernel",
             "knn_cells_scatter_kernel"]
    assert rec["cells_S300"] == build + ["knn_cells_search_kernel<8>"]
    assert rec["cells_S0"] == [n for n in build if n != "knn_cells_bounds_kernel"] + ["knn_cells_search_kernel<4>"]
    assert not any("knn_search_kernel" in n or "knn_finish_kernel" in n for n in rec["cells_S300"] + rec["cells_S0"])
    # the brute-force call: what it listed before the second search existed (two spans at 300 sources; no span at none)
    assert rec["brute_S300"] == ["knn_search_kernel<8>", "knn_finish_kernel<8>"] and rec["brute_S0"] == ["knn_finish_kernel<4>"]


def test_the_entry_refuses_what_the_brute_force_entry_refuses(rec):
    assert rec["sizes"][:5] == [0] * 5 and rec["sizes"][5] > 0 and rec["sizes"][6] % 8 == 0
    assert rec["codes"] == [code for _, _, code in WRONG], list(zip([w for w, _, _ in WRONG], rec["codes"]))
    assert rec["good"] == [0, 0, 0, 0]


# ---- the public interface ---------------------------------------------------------------------------------------

def _field(T=5, S=60, seed=4):
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = (np.sin(5 * coords[:, 0])[None, :] + rs.standard_normal((T, S)) * 0.2).astype(np.float32)
    code = rs.randint(0, 4, size=(T, S))
    return coords, z, [code == c for c in (1, 2, 3)]


def test_an_unknown_search_is_refused_and_the_host_route_ignores_the_key():
    from stnf.utils import baselines as BL
    coords, z, masks = _field()
    assert BL.SEARCHES == ("brute", "cells")
    for bad in ("tree", "", None, 1):
        with pytest.raises(ValueError, match="search"):
            BL.grid_baselines(z, coords, *masks, config={"baseline_search": bad})
        with pytest.raises(ValueError, match="search"):
            BL.rasterize_nearest(coords, z[0], resolution=8, search=bad)
        with pytest.raises(ValueError, match="search"):
            BL.device_knn(None, None, None, 1, False, search=bad)
    plain = BL.grid_baselines(z, coords, *masks)
    for search in BL.SEARCHES:
        np.testing.assert_equal(BL.grid_baselines(z, coords, *masks, config={"baseline_search": search}), plain)
        for a, b in zip(BL.rasterize_nearest(coords, z[0], resolution=8, search=search),
                        BL.rasterize_nearest(coords, z[0], resolution=8)):
            assert kc.same_bits(a, b)


if __name__ == "__main__":
    drive()
