"""What the conformal tests rest on, checked without a GPU: the generated cases hold what they promise; the numpy
restatement of the radix select equals np.sort at every rank; the rank rule at exact products, at the textbook sizes
and beyond n; the exact identity that stands in for a statistical test (tie-free scores: coverage of the calibration
segment under its own offset is k / n); the comparators of tests/test_gpu_conformal.py fail four planted mistakes; the
host path of grid_scores with `conformal: true` and its untouched output without; the ABI in header, binding and
library; and, in a child process under STDADK_DRY_RUN=1 (validates and plans, launches nothing), the entry points
score_grid / conformal_grid call and every refusal of the two entry points.

This file is its own driver: `python tests/test_conformal_cases_cpu.py` with STDADK_DRY_RUN=1 prints the record."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from golden import conformal_cases as cc      # noqa: E402

C_TYPES = {"const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "const uint8_t *": ctypes.c_void_p,
           "void *": ctypes.c_void_p, "int64_t *": ctypes.c_void_p, "int32_t *": ctypes.c_void_p,
           "const int64_t *": ctypes.c_void_p, "const int32_t *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
           "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t,
           "stdadk_stream_t": ctypes.c_void_p}


# ------------------------------------------------------------------------------------------------ the cases
def test_constants_are_the_kernels_and_the_modules():
    from stnf import calibration as CF
    src = open(os.path.join(ROOT, "st-dadk_amd", "csrc", "conformal.hip")).read()
    assert int(re.search(r"constexpr int CS_RUN = (\d+);", src).group(1)) == cc.RUN
    assert int(re.search(r"constexpr int SEL_BITS = (\d+)", src).group(1)) == cc.SELECT_BITS == CF.SELECT_BITS
    assert (CF.RESID, CF.CQR, CF.ABS) == (cc.RESID, cc.CQR, cc.ABS)
    assert (CF.MAX_COLS, CF.MAX_SEGMENTS, CF.MAX_SELECT) == (cc.MAX_COLS, cc.MAX_SEGMENTS, cc.MAX_SELECT)


def test_score_cases_hold_what_the_generator_promises():
    assert cc.SCORE_S == [1, 63, 64, 65, 255, 256, 257, 513] and cc.SCORE_T == [1, 3, 4, 5, 16, 17, 33]
    assert cc.SCORE_Q == [1, 3, 5, 8] and cc.CODE_POOL == [0, 1, 2, 3, 7]
    seen = set()
    for S in cc.SCORE_S:
        for nT in cc.SCORE_T:
            for Q in cc.SCORE_Q:
                y, z, code = cc.make_score_case(S, nT, Q)
                assert y.shape == (nT * S, Q) and z.shape == code.shape == (nT, S)
                assert y.dtype == z.dtype == np.float32 and code.dtype == np.uint8 and np.isfinite(y).all()
                assert set(np.unique(code)) <= set(cc.CODE_POOL)
                cond = cc.conditions(y, z, code)
                for key in cc.promised(S, nT):
                    assert cond[key], (S, nT, Q, key)
                    seen.add(key)
                assert len(cc.score_cols(Q)) <= cc.MAX_COLS
    assert seen == {"nan", "pinf", "ninf", "other_code", "empty_slice", "full_slice", "empty_run", "full_run"}
    y, z, code = cc.make_score_case(257, 33, 5)
    assert (cc.conditions(y, z, code)["members"] > cc.RUN).all()          # both segments span several runs


def test_key_cases_hold_what_the_generator_promises():
    assert cc.KEY_N == [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65537, 1048579]
    assert len(cc.FAMILIES) == 9
    for fam in cc.FAMILIES:
        for n in cc.KEY_N[:-1]:
            x = cc.make_keys(fam, n)
            assert x.shape == (n,) and x.dtype == np.float32 and np.isfinite(x).all(), (fam, n)
    bits = lambda fam: cc.make_keys(fam, 65537).view(np.uint32)      # noqa: E731
    assert len(np.unique(cc.make_keys("equal", 65537))) == 1 and len(np.unique(cc.make_keys("two", 65537))) == 2
    assert len(np.unique(cc.make_keys("seven", 65537))) == 7
    assert len(np.unique(bits("low_byte") >> 8)) == 1 and len(np.unique(bits("low_byte") & 0xFF)) == 256
    assert len(np.unique(bits("top_byte") & 0xFFFFFF)) == 1 and len(np.unique(bits("top_byte") >> 24)) == 256
    z = cc.make_keys("zeros", 65537)
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    d = cc.make_keys("denormal", 65537)
    assert (np.abs(d) < np.finfo(np.float32).tiny).all() and (d != 0).all() and (d < 0).any() and (d > 0).any()
    m = cc.make_keys("fltmax", 65537)
    assert (m == cc.FLT_MAX).any() and (m == -cc.FLT_MAX).any()
    u = cc.make_keys("uniform", 65537)
    assert (u < 0).any() and (u > 0).any()
    assert cc.ranks(257) == list(range(257)) and cc.ranks(1025) == [0, 1, 512, 1023, 1024]


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_select_restatement_is_np_sort_at_every_rank(family):
    from stnf import calibration as CF
    for n in [n for n in cc.KEY_N if n <= cc.SMALL_N]:
        x = cc.make_keys(family, n)
        s = np.sort(x)
        for k in range(n):
            v, used = CF.select_numpy(x, k)
            assert v == s[k] and used == k and v.dtype == np.float32, (family, n, k)
    x = cc.make_keys(family, 65537)
    s = np.sort(x)
    for k in cc.ranks(65537):
        assert CF.select_numpy(x, k)[0] == s[k]
    assert CF.select_numpy(x, 65537) == (np.inf, -1) and CF.select_numpy(x[:0], 0) == (np.inf, -1)


def test_key_map_preserves_order_and_inverts():
    from stnf import calibration as CF
    x = np.concatenate([cc.make_keys(f, 1025) for f in cc.FAMILIES])
    k = CF.select_keys(x)
    order = np.argsort(k, kind="stable")
    assert (np.diff(x[order]) >= 0).all()
    back = CF.select_values(k)
    assert np.array_equal(back, x) and not np.signbit(back[x == 0]).any()            # -0 comes back as +0
    assert CF.select_keys(np.float32([-0.0]))[0] == CF.select_keys(np.float32([0.0]))[0] == 0x80000000


def test_rank_rule():
    from stnf import calibration as CF
    # (n + 1) beta an exact integer: the ceiling must not step past it
    for n, beta, k in ((1, 0.5, 1), (3, 0.5, 2), (7, 0.5, 4), (3, 0.75, 3), (7, 0.75, 6), (99, 0.5, 50), (1023, 0.75, 768)):
        assert CF.conformal_rank(n, beta) == k - 1, (n, beta)
    # the textbook sizes at 90 %: the largest score at n = 9, the 18th of 19, the 90th of 99
    assert [CF.conformal_rank(n, 0.9) for n in (9, 19, 99)] == [8, 17, 89]
    # not enough calibration data
    assert CF.conformal_rank(8, 0.9) == -1 and CF.conformal_rank(0, 0.5) == -1 and CF.conformal_rank(0, 0.0) == -1
    assert CF.conformal_rank(5, 1.0) == -1 and CF.conformal_rank(5, 0.0) == 0            # k below 1 is taken as 1
    assert CF.interval_beta(0.1) == 1.0 - 0.1 and CF.level_beta(0.25) == 0.25
    x = cc.make_keys("uniform", 19)
    assert CF.select_level_numpy(x, 0.9) == (np.sort(x)[17], 17)
    assert CF.select_level_numpy(x[:8], 0.9) == (np.inf, -1)


def test_coverage_of_the_calibration_segment_under_its_own_offset_is_k_over_n():
    """Tie-free scores: exactly k of the n calibration scores are <= the k-th smallest."""
    from stnf import calibration as CF
    rs = np.random.RandomState(5)
    for n in (9, 19, 64, 257, 1000):
        pred = np.sort(rs.standard_normal((n, 3)).astype(np.float32), axis=1)
        y = rs.standard_normal(n).astype(np.float32)
        plan = CF.make_plan(3, [0.1, 0.5, 0.9], [(0.1, 0.9)], 0.2)
        seg = CF.scores_numpy(pred, y, None, plan.cols, [0, 0])
        assert all(len(np.unique(row)) == n for row in seg[0])
        fin = CF.finish_host(plan, seg)                                  # evaluation segment = the calibration segment
        for j, (col, _, beta) in enumerate(plan.sels):
            k = CF.conformal_rank(n, beta) + 1
            assert fin["rank_used"][j] == k - 1 and fin["after"][j] == k, (n, j)
        rep = CF.report(plan, fin)
        assert rep["intervals"][0]["coverage_after"] == (CF.conformal_rank(n, 0.8) + 1) / n
        assert rep["n_cal"] == rep["n_eval"] == n and not rep["rank_beyond_n"] and rep["overflow"] == [False, False]


def test_scores_restatement_is_mask_order_float32():
    from stnf import calibration as CF
    y, z, code = cc.make_score_case(65, 5, 3)
    cols = cc.score_cols(3)
    seg = CF.scores_numpy(y, z, code, cols, cc.SEGMENT_CODES)
    for g, c in enumerate(cc.SEGMENT_CODES):
        m = (np.isfinite(z) & (code == c)).reshape(-1)
        zz = z.reshape(-1)
        assert seg[g].dtype == np.float32 and seg[g].shape == (len(cols), m.sum())
        assert np.array_equal(seg[g][0], (zz - y[:, 0])[m])
        assert np.array_equal(seg[g][3], np.maximum(y[:, 0] - zz, zz - y[:, 2])[m])
        assert np.array_equal(seg[g][4], np.abs(zz - y[:, 1])[m])


# ------------------------------------------------------------------------------------------------ the comparators
def test_the_comparators_fail_four_planted_mistakes():
    from stnf import calibration as CF
    x = cc.make_keys("uniform", 257)
    assert len(np.unique(x)) == 257 and (x < 0).sum() > 2
    s = np.sort(x)
    for k in (0, 100, 256):
        assert cc.compare_select(x, k, *CF.select_numpy(x, k)) == []
    assert cc.compare_select(x, 257, np.float32(np.inf), -1) == [] and cc.compare_select(x, 257, s[256], 256)
    # 1: rank off by one
    assert cc.compare_select(x, 100, s[101], 100) and cc.compare_select(x, 100, s[99], 100)
    assert cc.compare_select(x, 100, s[100], 101)
    # 2: negatives in the wrong order -- the sign bit flipped for every value, negatives not inverted
    wrong = x[np.argsort(x.view(np.uint32) ^ np.uint32(0x80000000), kind="stable")]
    assert any(cc.compare_select(x, k, wrong[k], k) for k in range(257))
    assert cc.compare_select(x, 0, wrong[0], 0)
    # 4: a tie run counted once
    t = cc.make_keys("seven", 257)
    uniq = np.unique(t)
    assert cc.compare_select(t, 100, uniq[min(100, len(uniq) - 1)], 100)
    assert cc.compare_select(t, 3, uniq[3], 3) and cc.compare_select(t, 100, np.sort(t)[100], 100) == []
    # 3: a dropped segment entry (and the honest segments pass, -0 and +0 told apart)
    y, z, code = cc.make_score_case(65, 5, 3)
    ref = CF.scores_numpy(y, z, code, cc.score_cols(3), cc.SEGMENT_CODES)
    cap = max(r.shape[1] for r in ref) + 3
    C = len(cc.score_cols(3))
    buf = np.full((2, C, cap), 7.0, dtype=np.float32)
    for g, r in enumerate(ref):
        buf[g, :, :r.shape[1]] = r
    count = [r.shape[1] for r in ref]
    assert cc.compare_segments(buf, count, ref) == []
    dropped = buf.copy()
    dropped[1, :, 5:-1] = buf[1, :, 6:]
    assert cc.compare_segments(dropped, count, ref) and cc.compare_segments(dropped, [count[0], count[1] - 1], ref)
    swapped = buf.copy()
    swapped[0, :, [2, 3]] = buf[0, :, [3, 2]]
    assert cc.compare_segments(swapped, count, ref)
    signed = buf.copy()
    signed[0, 0, 0] = -0.0
    ref0 = [r.copy() for r in ref]
    ref0[0][0, 0] = 0.0
    assert cc.compare_segments(signed, count, ref0)
    assert cc.compare_segments(buf, [4, 4], ref, cap=4) == [] and cc.compare_segments(buf, count, ref, cap=4)


# ------------------------------------------------------------------------------------------------ the host path
def _cpu_model(quantiles=True):
    return cc.e2e_model(quantiles=quantiles)


def _masks(code):
    return [code == c for c in (1, 2, 3)]


def test_grid_scores_host_path_and_untouched_output_without_the_key(tmp_path):
    from stnf import calibration as CF
    from stnf.utils import grid_scores
    from stnf.utils.predictions import save_grid_scores_npz
    m = _cpu_model()
    coords, z, code = cc.e2e_field()
    config = {"regression_type": "multi-quantile", "quantile_levels": cc.E2E_LEVELS, "interval": cc.E2E_INTERVAL}
    plain = grid_scores(m, z, coords, *_masks(code), config=config)
    off = grid_scores(m, z, coords, *_masks(code), config=dict(config, conformal=False))
    got = grid_scores(m, z, coords, *_masks(code), config=dict(config, conformal=True))
    assert "conformal" not in plain and set(off) == set(plain) and set(got) == set(plain) | {"conformal"}

    def same(a, b, where):
        assert type(a) is type(b), where
        if isinstance(a, dict):
            assert list(a) == list(b), where
            for k in a:
                same(a[k], b[k], where + (k,))
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b, equal_nan=True), where
        else:
            assert a == b or (a != a and b != b), where
    for other in (off, {k: v for k, v in got.items() if k != "conformal"}):
        same(plain, other, ())
    # the entry against the restatements applied by hand
    tv = cc.grid_times(cc.E2E_T)
    with torch.no_grad():
        pred = torch.stack([m(torch.zeros(cc.E2E_S, 0), torch.from_numpy(coords), torch.full((cc.E2E_S, 1), float(t)))
                            for t in tv]).numpy()
    cf = got["conformal"]
    assert cf["alpha"] == cc.E2E_ALPHA and cf["split"] == "valid"           # the interval's nominal miscoverage
    fin = np.isfinite(z)
    cal, ev = fin & (code == 2), fin & (code == 3)
    assert cf["n_cal"] == cal.sum() and cf["n_eval"] == ev.sum() and cf["overflow"] == [False, False]
    lo, hi = 0, 2
    s_cal = np.maximum(pred[:, :, lo] - z, z - pred[:, :, hi])[cal]
    s_ev = np.maximum(pred[:, :, lo] - z, z - pred[:, :, hi])[ev]
    k = CF.conformal_rank(cal.sum(), 1.0 - cc.E2E_ALPHA)
    iv = cf["intervals"][0]
    assert iv["offset"] == np.sort(s_cal)[k] and iv["rank_used"] == k and iv["n_cal"] == cal.sum()
    assert iv["coverage_before"] == (s_ev <= 0).mean() == plain["splits"]["test"]["coverage"]
    assert iv["coverage_after"] == (s_ev <= iv["offset"]).mean()
    assert abs(iv["mean_width_before"] - plain["splits"]["test"]["mean_width"]) < 1e-6
    assert iv["mean_width_after"] == iv["mean_width_before"] + 2.0 * iv["offset"]
    for q, tau in enumerate(cc.E2E_LEVELS):
        r_cal, r_ev = (z - pred[:, :, q])[cal], (z - pred[:, :, q])[ev]
        kq = CF.conformal_rank(cal.sum(), tau)
        assert cf["levels"]["offset"][q] == np.sort(r_cal)[kq] and cf["levels"]["rank_used"][q] == kq
        assert cf["levels"]["reliability_before"][q] == (r_ev <= 0).mean()
        assert cf["levels"]["reliability_after"][q] == (r_ev <= cf["levels"]["offset"][q]).mean()
    # apply: the widened interval holds exactly the evaluation entries the report counts (float32 on both sides)
    record = cf["calibration"]
    wide = record.apply(pred, cc.E2E_INTERVAL)
    assert wide.dtype == np.float32 and np.array_equal(wide[:, :, 1], pred[:, :, 1])
    inside = ((wide[:, :, lo] <= z) & (z <= wide[:, :, hi]))[ev].mean()
    assert abs(inside - iv["coverage_after"]) <= 1.0 / ev.sum()              # a score within an ulp of the offset
    shifted = record.apply(torch.from_numpy(pred))
    assert torch.equal(shifted, torch.from_numpy(pred + record.level_offsets))
    with pytest.raises(ValueError):
        record.apply(pred, (0.1, 0.5))
    # the record survives the file, and grid_scores.npz carries it
    back = CF.load_calibration_npz(CF.save_calibration_npz(tmp_path, record))
    for name in CF._NPZ:
        a, b = np.asarray(getattr(back, name)), np.asarray(getattr(record, name))
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name
    with np.load(save_grid_scores_npz(tmp_path, got)) as f:
        assert np.array_equal(f["conformal/interval_offsets"], record.interval_offsets)
    # too few calibration entries for this alpha: reported, not hidden
    few = grid_scores(m, z, coords, *_masks(code), config=dict(config, conformal=True, conformal_alpha=1e-4))
    assert few["conformal"]["rank_beyond_n"] and np.isposinf(few["conformal"]["intervals"][0]["offset"])
    assert few["conformal"]["intervals"][0]["rank_used"] == -1 and few["conformal"]["intervals"][0]["coverage_after"] == 1.0
    with pytest.raises(ValueError):
        grid_scores(m, z, coords, *_masks(code), config=dict(config, conformal=True, conformal_split="test"))


def test_grid_scores_host_path_of_a_mean_model():
    from stnf import calibration as CF
    from stnf.utils import grid_scores
    m = _cpu_model(quantiles=False)
    coords, z, code = cc.e2e_field()
    got = grid_scores(m, z, coords, *_masks(code), config={"conformal": True, "conformal_split": "train"})
    cf = got["conformal"]
    assert cf["alpha"] == 0.1 and cf["split"] == "train" and "levels" not in cf and "intervals" not in cf
    tv = cc.grid_times(cc.E2E_T)
    with torch.no_grad():
        pred = torch.stack([m(torch.zeros(cc.E2E_S, 0), torch.from_numpy(coords), torch.full((cc.E2E_S, 1), float(t)))
                            for t in tv]).numpy()[:, :, 0]
    fin = np.isfinite(z)
    a_cal, a_ev = np.abs(z - pred)[fin & (code == 1)], np.abs(z - pred)[fin & (code == 3)]
    k = CF.conformal_rank(a_cal.size, 0.9)
    assert cf["abs"]["half_width"] == np.sort(a_cal)[k] and cf["abs"]["coverage"] == (a_ev <= np.sort(a_cal)[k]).mean()
    band = cf["calibration"].apply(pred[:, :, None])
    c = np.float32(cf["abs"]["half_width"])
    assert band.shape == pred.shape + (2,) and np.array_equal(band[..., 0], pred - c) and np.array_equal(band[..., 1], pred + c)


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_library_agree():
    from stnf import _native as N
    hdr = open(os.path.join(ROOT, "include", "stdadk.h")).read()
    assert int(re.search(r"#define\s+STDADK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == N.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, res in (("stdadk_conformal_scores_f32", ctypes.c_int), ("stdadk_select_f32", ctypes.c_int),
                     ("stdadk_conformal_scores_workspace_bytes", ctypes.c_size_t),
                     ("stdadk_select_workspace_bytes", ctypes.c_size_t)):
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % sym, code, flags=re.S).group(1)
        want = [C_TYPES[re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()] for a in args.split(",")]
        got_res, got_args = N._SIGNATURES[sym]
        assert got_res is res and sym in N.exported_symbols()
        assert [ctypes.c_void_p if a not in (ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t) else a
                for a in got_args] == want, sym
        assert hasattr(ctypes.CDLL(N.LIB_PATH), sym) and hasattr(N.lib(), sym)
    for name, mine in (("CONFORMAL_RESID", cc.RESID), ("CONFORMAL_CQR", cc.CQR), ("CONFORMAL_ABS", cc.ABS),
                       ("CONFORMAL_MAX_COLS", cc.MAX_COLS), ("CONFORMAL_MAX_SEGMENTS", cc.MAX_SEGMENTS),
                       ("SELECT_MAX", cc.MAX_SELECT)):
        assert int(re.search(r"#define\s+STDADK_%s\s+(\d+)" % name, hdr).group(1)) == getattr(N, name) == mine
    assert "conformal" in open(os.path.join(ROOT, "st-dadk_amd", "csrc", "build.sh")).read()
    assert N.lib().stdadk_select_workspace_bytes(0) == 0 == N.lib().stdadk_select_workspace_bytes(17)
    assert N.lib().stdadk_select_workspace_bytes(1) == N.lib().stdadk_select_workspace_bytes(16) > 0
    assert N.lib().stdadk_conformal_scores_workspace_bytes(1 << 20, 1 << 12) == 0
    assert N.lib().stdadk_conformal_scores_workspace_bytes(1025, 1) == 2 * 2 * 8


# ------------------------------------------------------------------------------------------------ the dry run
SCORE_REFUSALS = {            # name: (keyword overrides of the honest call, the code)
    "neg_size": (dict(S=-1), -1), "Q0": (dict(Q=0), -1), "Q9": (dict(Q=9), -1), "C0": (dict(C=0), -1),
    "C9": (dict(C=9), -1), "G0": (dict(G=0), -1), "G3": (dict(G=3), -1), "kind": (dict(cols=[(3, 0, 0)]), -1),
    "col_a": (dict(cols=[(0, 3, 0)]), -1), "col_b": (dict(cols=[(1, 0, 3)]), -1), "code": (dict(codes=[2, 256]), -1),
    "neg_cap": (dict(cap=-1), -1), "null_cols": (dict(cols=None), -1), "null_codes": (dict(codes=None), -1),
    "null_count": (dict(count=0), -1), "null_overflow": (dict(overflow=0), -1), "null_scores": (dict(scores=0), -1),
    "null_y": (dict(y=0), -1), "null_z": (dict(z=0), -1), "null_ws": (dict(ws=0), -1),
    "rows": (dict(S=1 << 20, nT=1 << 12), -2), "cap31": (dict(cap=1 << 31), -2),
    "count_align": (dict(count=+4), -3), "scores_align": (dict(scores=+2), -3), "ws_align": (dict(ws=+4), -3),
    "ws_small": (dict(ws_bytes=-8), -4),
}
SELECT_REFUSALS = {
    "n_sel0": (dict(n_sel=0), -1), "n_sel17": (dict(n_sel=17), -1), "C0": (dict(C=0), -1), "C9": (dict(C=9), -1),
    "col": (dict(cols=[0, 2]), -1), "no_beta": (dict(ranks=[-1, 3], betas=None), -1),
    "beta_hi": (dict(ranks=[-1, 3], betas=[1.5, 0.0]), -1), "beta_nan": (dict(ranks=[-1, 3], betas=[float("nan"), 0.0]), -1),
    "neg_n_max": (dict(n_max=-1), -1), "null_keys": (dict(keys=0), -1), "null_n": (dict(n=0), -1),
    "null_value": (dict(value=0), -1), "null_rank_used": (dict(rank_used=0), -1), "null_ws": (dict(ws=0), -1),
    "null_sel": (dict(cols=None, n_sel=2), -1),
    "n_max31": (dict(n_max=1 << 31, stride=1 << 31), -2), "stride": (dict(stride=99), -2),
    "n_align": (dict(n=+4), -3), "keys_align": (dict(keys=+2), -3), "ws_align": (dict(ws=+4), -3),
    "ws_small": (dict(ws_bytes=-8), -4),
}


def _record():
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    from stnf import _native as N
    from stnf.engine import Predictor
    lib = N.lib()
    rec = {"scores": {}, "select": {}}
    buf = torch.zeros(1 << 16, dtype=torch.float64)                     # one honest buffer behind every pointer
    base = buf.data_ptr()

    def ptr(v):                # 0: NULL, +k: misaligned by k bytes, None: the buffer
        return None if v == 0 else base + (v or 0)

    def scores_call(S=100, nT=3, Q=3, cols=((0, 0, 0), (1, 0, 2)), C=None, codes=(2, 3), G=None, cap=50, y=None, z=None,
                    scores=None, count=None, overflow=None, ws=None, ws_bytes=0):
        flat = None if cols is None else (ctypes.c_int32 * (3 * len(cols)))(*[v for c in cols for v in c])
        cd = None if codes is None else (ctypes.c_int32 * len(codes))(*codes)
        need = lib.stdadk_conformal_scores_workspace_bytes(100, 3)
        rc = lib.stdadk_conformal_scores_f32(ptr(y), ptr(z), None, S, nT, Q, flat, len(cols or ()) if C is None else C, cd,
                                             len(codes or ()) if G is None else G, ptr(scores), cap, ptr(count),
                                             ptr(overflow), ptr(ws), need + ws_bytes, None)
        return [rc, lib.stdadk_last_error().decode()]

    def select_call(n_sel=None, C=2, cols=(0, 1), ranks=(0, -1), betas=(0.0, 0.9), stride=100, n_max=100, keys=None,
                    n=None, value=None, rank_used=None, ws=None, ws_bytes=0):
        k = len(cols or ()) if n_sel is None else n_sel
        arr = lambda t, v: None if v is None else (t * len(v))(*v)      # noqa: E731
        need = lib.stdadk_select_workspace_bytes(2)
        rc = lib.stdadk_select_f32(ptr(keys), stride, C, ptr(n), n_max, arr(ctypes.c_int32, cols),
                                   arr(ctypes.c_int64, ranks), arr(ctypes.c_double, betas), k, ptr(value),
                                   ptr(rank_used), ptr(ws), need + ws_bytes, None)
        return [rc, lib.stdadk_last_error().decode()]

    rec["scores"]["ok"], rec["select"]["ok"] = scores_call(), select_call()
    rec["scores"]["empty"] = scores_call(S=0, y=0, z=0, ws=0)
    for name, (kw, _) in SCORE_REFUSALS.items():
        rec["scores"][name] = scores_call(**kw)
    for name, (kw, _) in SELECT_REFUSALS.items():
        rec["select"][name] = select_call(**kw)

    # the entry points and kernels the Python face reaches: score_grid without and with a pass, conformal_grid
    real, log = lib, []

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.endswith("_f32") or name.startswith("stdadk_profile"):
                return fn

            def call(*args):
                log.append(name.replace("stdadk_", ""))
                return fn(*args)
            return call
    N.lib = lambda: Proxy()
    m = cc.e2e_model()
    coords, z, code = cc.e2e_field()
    ct, tv, zt, codet = (torch.from_numpy(a) for a in (coords, cc.grid_times(cc.E2E_T), z, code))
    pr = Predictor(m)
    kw = dict(split=codet, quantile_levels=cc.E2E_LEVELS, interval=cc.E2E_INTERVAL, max_rows=cc.E2E_MAX_ROWS)
    pr.score_grid(ct, tv, zt, **kw)
    rec["score_grid"] = list(log)
    del log[:]
    cf = pr.conformal_pass(700, cc.E2E_LEVELS, [cc.E2E_INTERVAL], cc.E2E_ALPHA)
    pr.score_grid(ct, tv, zt, quantile=True, conformal=cf, **kw)
    rec["score_grid_with_pass"] = list(log)
    del log[:]
    N.profile_enable(True)
    N.profile_collect()
    out = pr.conformal_grid(ct, tv, zt, codet, cc.E2E_LEVELS, [cc.E2E_INTERVAL], cc.E2E_ALPHA, max_rows=cc.E2E_MAX_ROWS,
                            cap=700)
    rec["conformal_grid"] = list(log)
    rec["conformal_kernels"] = [k for k, _ in N.profile_collect() if "conformal" in k or "select" in k]
    N.profile_enable(False)
    rec["conformal_keys"] = sorted(out)
    return rec


_RECORD = []


@pytest.fixture
def rec():
    if not _RECORD:
        env = dict(os.environ, STDADK_DRY_RUN="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        _RECORD.append(json.loads(r.stdout.splitlines()[-1]))
    return _RECORD[0]


def test_every_refusal_of_the_two_entry_points(rec):
    assert rec["scores"]["ok"][0] == 0 and rec["select"]["ok"][0] == 0 and rec["scores"]["empty"][0] == 0
    for table, who, word in ((SCORE_REFUSALS, "scores", "conformal_scores"), (SELECT_REFUSALS, "select", "select")):
        for name, (_, code) in table.items():
            rc, msg = rec[who][name]
            assert rc == code and msg.startswith(word + ":"), (who, name, rc, msg)
    codes = {c for _, c in SCORE_REFUSALS.values()} & {c for _, c in SELECT_REFUSALS.values()}
    assert codes == {-1, -2, -3, -4}                                    # _ARG, _SHAPE, _ALIGN, _WORKSPACE, both entries


def test_calls_made_by_score_grid_and_conformal_grid(rec):
    chunks = -(-cc.E2E_T // 3)
    plain = rec["score_grid"]
    assert plain.count("grid_score_f32") == chunks and not any("conformal" in c or "select" in c for c in plain)
    both = rec["score_grid_with_pass"]
    assert both.count("conformal_scores_f32") == both.count("grid_score_f32") == both.count("quantile_diag_f32") == chunks
    assert "select_f32" not in both                                      # conformal_finish makes that call
    assert [c for c in both if c not in ("conformal_scores_f32", "quantile_diag_f32")] == plain   # one forward per chunk
    grid = rec["conformal_grid"]
    assert grid.count("conformal_scores_f32") == chunks and grid.count("select_f32") == 1 and grid[-1] == "select_f32"
    assert not any(c in ("grid_score_f32", "quantile_diag_f32") for c in grid)
    assert [c for c in grid if c not in ("conformal_scores_f32", "select_f32")] == \
        [c for c in plain if c != "grid_score_f32"]
    per_chunk = ["conformal_count_kernel", "conformal_scan_kernel", "conformal_scatter_kernel"]
    select = ["select_setup_kernel"] + ["select_hist_kernel", "select_pick_kernel"] * (32 // cc.SELECT_BITS)
    assert rec["conformal_kernels"] == per_chunk * chunks + select
    assert {"alpha", "calibration", "intervals", "levels", "n_cal", "n_eval", "overflow", "rank_beyond_n"} <= set(
        rec["conformal_keys"])


if __name__ == "__main__":
    print(json.dumps(_record()))
