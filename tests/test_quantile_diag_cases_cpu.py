"""The quantile-diagnostics cases of tests/golden/quantile_diag_cases.py, checked where no GPU is needed: that every
generated case holds what the generator promises, per split; that the restatement's DEPTH1 / N, DEPTH2 / N and CRPS / N
are the oracle's non_crossing_penalty, check_loss and crps (pinned on the reference); its invariants; that the
comparator of tests/test_gpu_quantile_diag.py fails the four mistakes such a reduction can make; the host path of
grid_scores with `quantile_diagnostics`; the ABI (header, binding, library, the kernel's constants); and, in a child
process under STDADK_DRY_RUN=1 (every entry point validates and plans, nothing is launched, host tensors), the calls of
score_grid with and without `quantile=True` and the refusals of stdadk_quantile_diag_f32.

This file is its own driver, like tests/test_grid_cases_cpu.py: `python tests/test_quantile_diag_cases_cpu.py` with
STDADK_DRY_RUN=1 prints the record as JSON."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from golden import quantile_diag_cases as qc           # noqa: E402
from oracle import stdadk_oracle as orc                # noqa: E402

U53 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("Q", range(1, qc.MAX_Q + 1))
def test_every_case_holds_what_the_generator_promises(Q):
    sizes, slices = qc.kernel_shapes(Q)
    assert sizes == [1, 63, 64, 65, 255, 256, 257, 513] and slices[-4:] == [15, 16, 17, 33]
    assert slices[:4] == ([1, 7, 8, 9] if Q <= 4 else [1, 3, 4, 5])
    big = 0
    for S in sizes:
        for nT in slices:
            y, z, code = qc.make_case(S, nT, Q)
            assert y.shape == (S * nT, Q) and z.shape == code.shape == (nT, S)
            assert y.dtype == z.dtype == np.float32 and code.dtype == np.uint8
            assert np.isfinite(y).all() and set(np.unique(code).tolist()) <= {0, 1, 2, 3, 7}
            if S * nT < 64:
                continue
            big += 1
            have = qc.conditions(y, z, code)
            assert 7 in have, (S, nT)
            for c in range(4):
                assert qc.required(Q) <= have[c], (S, nT, c, qc.required(Q) - have[c])
    assert big >= 50


def test_toggles_cover_every_combination():
    for Q in range(2, qc.MAX_Q + 1):
        assert len({qc.toggles(i, j, Q) for i in range(8) for j in range(8)}) == 16
    assert len({qc.toggles(i, j, 1) for i in range(8) for j in range(8)}) == 8      # Q == 1 has no interval


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("Q", [1, 2, 5, 8])
def test_restatement_agrees_with_the_pinned_oracle(Q):
    """Per split: DEPTH1 / N and DEPTH2 / N are non_crossing_penalty(rows, power, "mean"), CRPS / N is crps(rows, z,
    taus) = 2 mean_q check_loss.  Both sides are float64 sums of the same n Q products in other orders: within
    (n Q + 8) 2^-53 of the sum of magnitudes."""
    S, nT = 257, 17
    y, z, code = qc.make_case(S, nT, Q, seed=11)
    taus = qc.levels(Q).astype(np.float64)
    split = qc.restate(y, z, code, taus)[0]
    zf = z.reshape(-1)
    for c in range(4):
        m = np.isfinite(zf) & (code.reshape(-1) == c)
        n = int(m.sum())
        assert n == split[c, qc.N_] > 0
        rows, obs = y[m].astype(np.float64), zf[m].astype(np.float64)
        tol = (n * Q + 8) * U53
        for power, slot in ((1, qc.DEPTH1), (2, qc.DEPTH2)):
            ref = orc.non_crossing_penalty(rows, power=power, reduction="mean")
            assert abs(split[c, slot] / n - ref) <= tol * abs(ref), (c, power)
        ref = orc.crps(rows, obs, list(taus))
        mags = 2.0 * np.mean([orc.check_loss(rows[:, q], obs, taus[q]) for q in range(Q)])     # the terms are >= 0
        assert abs(split[c, qc.CRPS] / n - ref) <= tol * mags, c
        assert abs(ref - mags) <= tol * mags


def test_invariants():
    """sum_j PIT_j = N everywhere; on sorted rows z <= p_q exactly when fewer than q + 1 levels lie below z, so
    BELOW_q = sum_{j <= q} PIT_j."""
    for Q in (1, 3, 8):
        y, z, code = qc.make_case(65, 9, Q, seed=12)
        split, site, time = qc.restate(y, z, code, qc.levels(Q), 0 if Q > 1 else -1, Q - 1 if Q > 1 else -1)
        assert np.array_equal(split[:, qc.PIT:qc.PIT + Q + 1].sum(axis=1), split[:, qc.N_])
        for v in (qc.SV_N, qc.SV_CROSS, qc.SV_INSIDE):
            assert np.array_equal(site[:, :, v].sum(axis=1), time[:, :, v].sum(axis=1))
        assert np.array_equal(site[:, :, qc.SV_N].sum(axis=1), split[:, qc.N_])
        assert np.array_equal(site[:, :, qc.SV_CROSS].sum(axis=1), split[:, qc.CROSS_ROWS])
        assert np.array_equal(site[:, :, qc.SV_INSIDE].sum(axis=1), split[:, qc.INSIDE])
        ys = np.sort(y, axis=1)
        s2 = qc.restate(ys, z, code, qc.levels(Q))[0]
        assert np.array_equal(s2[:, qc.BELOW:qc.BELOW + Q], np.cumsum(s2[:, qc.PIT:qc.PIT + Q], axis=1))
        assert not s2[:, qc.CROSS_ROWS].any() and not s2[:, qc.DEPTH1].any() and not s2[:, qc.PAIR:qc.PAIR + Q].any()
        if Q > 1:
            assert (split[:, qc.CROSS_ROWS] > 0).all() and (split[:, qc.DEPTH2] > 0).all()
    # Q == 1: no pairs, two PIT bins
    y, z, code = qc.make_case(65, 9, 1, seed=13)
    s1 = qc.restate(y, z, code, qc.levels(1))[0]
    assert not s1[:, qc.CROSS_ROWS:qc.CRPS].any() and not s1[:, qc.PIT + 2:qc.CROSS_ROWS].any()


# ------------------------------------------------------------------------------------------------ the comparator's teeth
def test_comparator_passes_the_restatement_and_fails_four_mistakes():
    S, nT, Q = 65, 9, 5
    y, z, code = qc.make_case(S, nT, Q, seed=14)
    taus = qc.levels(Q)
    ref = qc.restate(y, z, code, taus, 0, Q - 1)
    bound = qc.bounds(y, z, code, taus, 0, Q - 1)
    assert not qc.compare(ref, ref, bound)
    # a sum inside its bound passes, one outside fails
    near = [a.copy() for a in ref]
    near[0][1, qc.CRPS] += 0.5 * bound[0][1, qc.CRPS]
    assert not qc.compare(near, ref, bound)
    near[0][1, qc.CRPS] += bound[0][1, qc.CRPS]
    assert qc.compare(near, ref, bound)
    mistakes = {
        "BELOW with <": qc.restate(y, z, code, taus, 0, Q - 1, below=np.less),
        "crossing with >=": qc.restate(y, z, code, taus, 0, Q - 1, crosses=np.greater_equal),
    }
    off = [a.copy() for a in ref]
    off[0][2, qc.PIT + 1] += 1
    mistakes["a count off by one"] = off
    moved = code.copy()
    ti, si = [(t, s) for t, s in zip(*np.nonzero(np.isfinite(z) & (code == 1)))][0]
    moved[ti, si] = 2
    mistakes["a row moved to another split"] = qc.restate(y, z, moved, taus, 0, Q - 1)
    for what, got in mistakes.items():
        bad = qc.compare(got, ref, bound)
        print(f"{what}: {len(bad)} differences, e.g. {bad[:1]}")
        assert bad, what
    # a site count off by one, a missing time slice
    off = [a.copy() for a in ref]
    off[1][3, 7, qc.SV_CROSS] += 1
    assert qc.compare(off, ref, bound)
    assert qc.compare((ref[0], ref[1], ref[2][:, :-1]), ref, bound)


# ------------------------------------------------------------------------------------------------ the host path
def _host_grid(m, coords, T):
    import torch
    S = len(coords)
    with torch.no_grad():
        return np.stack([m(torch.zeros(S, 0), torch.from_numpy(coords), torch.full((S, 1), float(t))).double().numpy()
                         for t in qc.grid_times(T)])


def test_e2e_model_has_crossing_and_sorted_rows_in_every_split():
    """The freshly initialised model of the end-to-end GPU tests, through its host path with the same seed."""
    m = qc.e2e_model()
    coords, z, code = qc.e2e_field()
    split = qc.restate(_host_grid(m, coords, qc.E2E_T), z, code, qc.E2E_LEVELS)[0]
    print("rows", split[:, qc.N_].tolist(), "crossing rows", split[:, qc.CROSS_ROWS].tolist())
    assert (split[:, qc.CROSS_ROWS] > 0).all() and (split[:, qc.CROSS_ROWS] < split[:, qc.N_]).all()
    assert np.isnan(z).sum() > 0 and (z == np.inf).sum() == 1 and (z == -np.inf).sum() == 1
    # the delta head as the tests build it never crosses
    md = qc.e2e_model(delta=True)
    sd = qc.restate(_host_grid(md, coords, qc.E2E_T), z, code, qc.E2E_LEVELS)[0]
    assert not sd[:, qc.CROSS_ROWS].any() and not sd[:, qc.DEPTH1].any()


def test_host_grid_scores_quantile_entry(tmp_path):
    """grid_scores(cpu model, quantile_diagnostics) equals the restatement applied to the model's own host predictions:
    counts exact; the float sums are numpy's own float64 sums of the same terms, within the derived bound on both sides.
    Without the key the dict has no `quantile` entry and is today's output."""
    import test_grid_scores_cpu as GSC
    from stnf.utils import grid_scores, save_grid_scores_npz
    m = qc.e2e_model()
    coords, z, code = qc.e2e_field()
    masks = [code == c for c in (1, 2, 3)]
    S, T, Q = qc.E2E_S, qc.E2E_T, len(qc.E2E_LEVELS)
    config = {"regression_type": "multi-quantile", "quantile_levels": qc.E2E_LEVELS, "interval": qc.E2E_INTERVAL}
    pred = _host_grid(m, coords, T)
    plain = grid_scores(m, z, coords, *masks, config=config)
    assert "quantile" not in plain
    finite_z = np.where(np.isfinite(z), z, np.nan)           # (the older oracle knows NaN only)
    with np.errstate(invalid="ignore"):
        GSC_S, GSC.S = GSC.S, S
        try:
            GSC.assert_scores(grid_scores(m, finite_z, coords, *masks, config=config),
                              GSC.oracle(pred, finite_z, code, qc.E2E_LEVELS, qc.E2E_INTERVAL), 1e-12)
        finally:
            GSC.S = GSC_S
    got = grid_scores(m, z, coords, *masks, config=dict(config, quantile_diagnostics=True))
    assert set(got) == set(plain) | {"quantile"}
    for k, v in plain.items():
        if k != "splits":
            assert np.array_equal(got[k], v, equal_nan=True), k
    assert got["splits"] == plain["splits"]
    # a mean model has no levels: the key changes nothing
    from stnf.models import STInterpMLP
    mean = STInterpMLP(p=0, k_spatial_centers=[9], k_temporal_centers=[5], hidden_dims=[16], dropout=0.0).eval()
    assert "quantile" not in grid_scores(mean, z, coords, *masks, config={"quantile_diagnostics": True})

    split, site, time = qc.restate(pred, z, code, qc.E2E_LEVELS, 0, Q - 1)
    bsplit, bsite, btime = qc.bounds(pred, z, code, qc.E2E_LEVELS, 0, Q - 1)
    qd = got["quantile"]
    assert set(qd) == {"all", "train", "valid", "test", "other", "site_crps", "site_cross_rate", "site_coverage",
                       "site_count", "site_crps_by_split", "time_crps", "time_cross_rate", "time_coverage", "time_count",
                       "time_crps_by_split"}
    rows = {"other": split[0], "train": split[1], "valid": split[2], "test": split[3], "all": split.sum(axis=0)}
    brow = {"other": bsplit[0], "train": bsplit[1], "valid": bsplit[2], "test": bsplit[3], "all": bsplit.sum(axis=0)}
    for name, r in rows.items():
        e, n = qd[name], r[qc.N_]
        assert set(e) == {"levels", "reliability", "pit", "cross_rate", "pair_cross_rate", "nc_penalty_p1",
                          "nc_penalty_p2", "crps", "rows", "coverage"}
        assert e["rows"] == n > 0 and list(e["levels"]) == qc.E2E_LEVELS
        assert e["reliability"].shape == (Q,) and e["pit"].shape == (Q + 1,) and e["pair_cross_rate"].shape == (Q - 1,)
        assert np.array_equal(e["reliability"], r[qc.BELOW:qc.BELOW + Q] / n)
        assert np.array_equal(e["pit"], r[qc.PIT:qc.PIT + Q + 1] / n)
        assert np.array_equal(e["pair_cross_rate"], r[qc.PAIR:qc.PAIR + Q - 1] / n)
        assert e["cross_rate"] == r[qc.CROSS_ROWS] / n and e["coverage"] == r[qc.INSIDE] / n
        for key, slot in (("nc_penalty_p1", qc.DEPTH1), ("nc_penalty_p2", qc.DEPTH2), ("crps", qc.CRPS)):
            # (two more roundings: the division here and the product below)
            assert abs(e[key] * n - r[slot]) <= 2 * brow[name][slot] + 4 * U53 * abs(r[slot]), (name, key)
    for name, acc, b in (("site", site, bsite), ("time", time, btime)):
        cnt = acc[:, :, qc.SV_N]
        assert np.array_equal(qd[f"{name}_count"], cnt.sum(axis=0))
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(qd[f"{name}_cross_rate"], acc[:, :, qc.SV_CROSS].sum(axis=0) / cnt.sum(axis=0),
                                  equal_nan=True)
            assert np.array_equal(qd[f"{name}_coverage"], acc[:, :, qc.SV_INSIDE].sum(axis=0) / cnt.sum(axis=0),
                                  equal_nan=True)
            ref = acc[:, :, qc.SV_CRPS] / cnt
            tol = (2 * b + 4 * U53 * np.abs(acc[:, :, qc.SV_CRPS])) / cnt
        by = qd[f"{name}_crps_by_split"]
        assert by.shape == cnt.shape and np.array_equal(np.isnan(by), cnt == 0)
        assert (np.abs(by - ref)[cnt > 0] <= tol[cnt > 0]).all()
        tot = acc[:, :, qc.SV_CRPS].sum(axis=0)
        ok = cnt.sum(axis=0) > 0
        assert (np.abs(qd[f"{name}_crps"] * cnt.sum(axis=0) - tot)[ok]
                <= (2 * b.sum(axis=0) + 8 * U53 * np.abs(tot))[ok]).all()
    # the npz record carries the new arrays, and none of them without the key
    back = np.load(save_grid_scores_npz(tmp_path / "with", got))
    assert np.array_equal(back["quantile/site_crps"], qd["site_crps"], equal_nan=True)
    assert np.array_equal(back["quantile/test/pit"], qd["test"]["pit"]) and back["quantile/all/rows"] == qd["all"]["rows"]
    assert not [k for k in np.load(save_grid_scores_npz(tmp_path / "without", plain)).files if k.startswith("quantile")]


# ------------------------------------------------------------------------------------------------ ABI
C_TYPES = {"const float *": ctypes.c_void_p, "const uint8_t *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "void *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t,
           "stdadk_stream_t": ctypes.c_void_p}


def _header():
    return open(os.path.join(ROOT, "include", "stdadk.h")).read()


def test_header_binding_library_and_cases_agree():
    from stnf import _native as N
    hdr = _header()
    assert int(re.search(r"#define\s+STDADK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == N.ABI_VERSION
    assert int(re.search(r"#define\s+STDADK_MAX_Q\s+(\d+)", hdr).group(1)) == qc.MAX_Q
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, res in (("stdadk_quantile_diag_f32", ctypes.c_int), ("stdadk_quantile_diag_workspace_bytes", ctypes.c_size_t)):
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % sym, code, flags=re.S).group(1)
        want = [C_TYPES[re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()] for a in args.split(",")]
        got_res, got_args = N._SIGNATURES[sym]
        assert got_res is res and sym in N.exported_symbols()
        assert [ctypes.c_void_p if a is ctypes.POINTER(ctypes.c_float) else a for a in got_args] == want, sym
        assert hasattr(ctypes.CDLL(N.LIB_PATH), sym)
    for name, mine in (("N", qc.N_), ("BELOW", qc.BELOW), ("PIT", qc.PIT), ("CROSS_ROWS", qc.CROSS_ROWS),
                       ("PAIR", qc.PAIR), ("DEPTH1", qc.DEPTH1), ("DEPTH2", qc.DEPTH2), ("CRPS", qc.CRPS),
                       ("INSIDE", qc.INSIDE), ("SLOTS", qc.SLOTS)):
        assert int(re.search(r"#define\s+STDADK_QD_%s\s+(\d+)" % name, hdr).group(1)) == getattr(N, "QD_" + name) == mine
    assert qc.SLOTS == 32 and sorted(qc.COUNT_SLOTS + qc.FLOAT_SLOTS) == list(range(30))
    # the constants the GPU test's shapes are named from
    csrc = os.path.join(ROOT, "st-dadk_amd", "csrc")
    red, kern = open(os.path.join(csrc, "grid_reduce.h")).read(), open(os.path.join(csrc, "quantile_diag.hip")).read()
    assert int(re.search(r"constexpr int GS_T = (\d+);", red).group(1)) == qc.SITES_PER_WG
    assert int(re.search(r"constexpr int QD_TT = (\d+);", kern).group(1)) == qc.TILE_SLICES
    u = re.search(r"constexpr int QD_U = Q <= (\d+) \? (\d+) : (\d+);", kern)
    assert [qc.load_unroll(q) for q in (int(u.group(1)), int(u.group(1)) + 1)] == [int(u.group(2)), int(u.group(3))]
    assert "quantile_diag" in open(os.path.join(csrc, "build.sh")).read()


# ------------------------------------------------------------------------------------------------ the dry-run driver
_NAMES = {"stdadk_forward_parts_f32": "forward_parts", "stdadk_forward_f32": "forward",
          "stdadk_grid_score_f32": "grid_score", "stdadk_quantile_diag_f32": "quantile_diag",
          "stdadk_spatial_partial_f32": "spatial_partial", "stdadk_temporal_partial_f32": "temporal_partial",
          "stdadk_gemm_f32": "gemm", "stdadk_rbf_build_f32": "rbf_build"}


def _record():
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    import torch
    from stnf import _native as N
    from stnf.engine import Predictor
    real = N.lib()
    rec = {}
    # ---- the entry point's refusals, through the library itself (no pointer is dereferenced in a dry run)
    S, nT, Q = 67, 3, 5
    need = real.stdadk_quantile_diag_workspace_bytes(S, nT)
    buf = torch.zeros(need // 8 + 2, dtype=torch.float64)
    ptr = buf.data_ptr()
    assert ptr % 8 == 0
    taus = (ctypes.c_float * 8)(*([0.5] * 8))

    def call(S=S, nT=nT, Q=Q, lo=0, hi=4, split_acc=ptr, site=ptr, time=ptr, ws=ptr, nbytes=need, taus=taus):
        rc = real.stdadk_quantile_diag_f32(ptr, ptr, None, S, nT, Q, taus, lo, hi, split_acc, site, time, ws, nbytes, None)
        return [rc, real.stdadk_last_error().decode() if rc else ""]
    rec["refusals"] = {
        "good": call(), "no_interval_no_levels": call(lo=-1, hi=-1, taus=None), "no_site_no_time": call(site=None, time=None),
        "Q0": call(Q=0, lo=-1, hi=-1), "Q9": call(Q=9), "lo_ge_hi": call(lo=3, hi=3), "half_interval": call(lo=-1, hi=2),
        "hi_past_Q": call(hi=5), "no_split_acc": call(split_acc=None), "negative": call(S=-1),
        "short_workspace": call(nbytes=need - 8), "misaligned_workspace": call(ws=ptr + 4),
        "too_large": call(S=1 << 16, nT=1 << 15), "empty": call(S=0)}
    rec["need"] = [need, real.stdadk_quantile_diag_workspace_bytes(1 << 16, 1 << 15),
                   real.stdadk_quantile_diag_workspace_bytes(S, 0)]
    # ---- the wrapper's own check of an accumulator: split_acc with grid_score's slots, not quantile_diag's
    try:
        N.quantile_diag(torch.zeros(nT * S, Q), torch.zeros(nT, S), None, None, -1, -1,
                        torch.zeros(4, N.GRID_SLOTS, dtype=torch.float64), None, None, buf)
        rec["wrong_split_acc"] = None
    except RuntimeError as e:
        rec["wrong_split_acc"] = str(e)
    # ---- the calls of score_grid / quantile_grid
    log = []

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in _NAMES:
                return fn

            def call(*args):
                log.append(_NAMES[name])
                return fn(*args)
            return call

    proxy = Proxy()
    N.lib = lambda: proxy
    coords, z, code = qc.e2e_field()
    tv = qc.grid_times(qc.E2E_T)
    args = tuple(torch.from_numpy(a) for a in (coords, tv, z, code))
    rec["grids"] = {}
    for route, spec in qc.ROUTES.items():
        m = qc.e2e_model(hidden=spec["hidden"])
        m.force_window_path = spec["force_window"]
        pr = Predictor(m, chunk=4096)
        uses_window = bool(N.step_uses_window(pr.state.basis, pr.state.desc, pr.state.flags))
        out = {}
        for key, fn in (("default", lambda **kw: pr.score_grid(*args, **kw)),
                        ("quantile", lambda **kw: pr.score_grid(*args, quantile=True, **kw)),
                        ("quantile_grid", lambda **kw: pr.quantile_grid(*args, **kw))):
            for max_rows in (None, 3 * qc.E2E_S + 5):
                del log[:]
                accs = fn(quantile_levels=qc.E2E_LEVELS, interval=qc.E2E_INTERVAL, max_rows=max_rows)
                out[f"{key}/{max_rows}"] = dict(calls=list(log), shapes=[list(a.shape) for a in accs])
        out["uses_window"] = uses_window
        rec["grids"][route] = out
    return rec


_RECORD = []


def _recorded():
    if not _RECORD:
        env = dict(os.environ, STDADK_DRY_RUN="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        _RECORD.append(json.loads(r.stdout))
    return _RECORD[0]


def test_entry_point_refusals_return_the_stated_codes():
    hdr = _header()
    E = {k: int(re.search(r"#define\s+STDADK_E_%s\s+\((-\d+)\)" % k, hdr).group(1))
         for k in ("ARG", "SHAPE", "ALIGN", "WORKSPACE")}
    rec = _recorded()
    ref = rec["refusals"]
    for key in ("good", "no_interval_no_levels", "no_site_no_time", "empty"):
        assert ref[key] == [0, ""], key
    for key, code, word in (("Q0", "ARG", "Q=0 outside 1..8"), ("Q9", "ARG", "Q=9 outside 1..8"),
                            ("lo_ge_hi", "ARG", "interval"), ("half_interval", "ARG", "interval"),
                            ("hi_past_Q", "ARG", "interval"), ("no_split_acc", "ARG", "NULL"),
                            ("negative", "ARG", "negative"), ("short_workspace", "WORKSPACE", "workspace"),
                            ("misaligned_workspace", "ALIGN", "aligned"), ("too_large", "SHAPE", "31 bits")):
        assert ref[key][0] == E[code] and word in ref[key][1], (key, ref[key])
    need, too_large, no_slices = rec["need"]
    assert need > 0 and need % 8 == 0 and too_large == 0 and no_slices > 0


def test_wrapper_names_itself_when_it_refuses_an_accumulator():
    """A split_acc of the wrong shape passed to _native.quantile_diag is reported as quantile_diag's, with the shape it
    wants, and not as grid_score's (the two wrappers once shared a check that named only grid_score)."""
    msg = _recorded()["wrong_split_acc"]
    assert msg is not None and msg.startswith("quantile_diag: split_acc must be") and "grid_score" not in msg, msg
    assert "of shape (4, 32)" in msg and "(4, 16)" in msg, msg


@pytest.mark.parametrize("route", ["window", "materialising", "expanded"])
def test_dry_run_one_forward_per_chunk_and_both_reductions_after_it(route):
    """score_grid(quantile=True) issues exactly one forward (forward_parts, or forward on the expanded route) per chunk
    of time slices, followed by grid_score and then quantile_diag on that chunk; the default issues today's calls -- the
    same list without the quantile_diag entries; quantile_grid the same list without the grid_score entries."""
    rec = _recorded()["grids"][route]
    S, T = qc.E2E_S, qc.E2E_T
    fwd = "forward" if route == "expanded" else "forward_parts"
    assert rec["uses_window"] == (route == "window")
    assert ("spatial_partial" in rec["default/None"]["calls"]) == (route == "window")
    assert ("gemm" in rec["default/None"]["calls"]) == (route == "materialising")
    for max_rows, chunks in ((None, 1), (3 * S + 5, -(-T // 3))):
        d, q, g = (rec[f"{k}/{max_rows}"] for k in ("default", "quantile", "quantile_grid"))
        assert d["shapes"] == [[4, 16], [4, S, 3], [4, T, 3]]
        assert q["shapes"] == d["shapes"] + [[4, 32], [4, S, 4], [4, T, 4]] and g["shapes"] == q["shapes"][3:]
        assert [c for c in q["calls"] if c != "quantile_diag"] == d["calls"]
        assert [c for c in q["calls"] if c != "grid_score"] == g["calls"]
        assert "quantile_diag" not in d["calls"] and d["calls"].count("grid_score") == chunks
        tail = q["calls"][q["calls"].index(fwd):]
        assert tail == [fwd, "grid_score", "quantile_diag"] * chunks, (route, max_rows, tail)
        assert q["calls"].count(fwd) == chunks


if __name__ == "__main__":
    json.dump(_record(), sys.stdout)
    sys.exit(0)
