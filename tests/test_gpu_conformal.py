"""Conformal calibration on the device.  stdadk_conformal_scores_f32 through the ABI on the generated cases of
tests/golden/conformal_cases.py: both segments BIT-identical to numpy float32 arithmetic in numpy's mask order, chunked
calls against one call, a capacity below the member count.  stdadk_select_f32: equal by value to np.sort at every rank
(n <= 257) or at {0, 1, n/2, n - 2, n - 1}, every value family, eight columns behind a stride, sixteen selections,
levels, n from the scores call's counter, twice the same bits, under graph capture.  Then end to end on a tiny model:
Predictor.conformal_grid equals the numpy restatement of predict_grid's own output, grid_scores with and without the
key, the Evaluator path, and Calibration.apply shown by the quantile diagnostics."""
import numpy as np
import pytest
import torch

from golden import conformal_cases as cc
import test_gpu_parity as T

pytestmark = pytest.mark.gpu
GUARD = 7.25                                   # what fills the score buffers before a call


def run_scores(y, z, code, cols, codes, cap, scores=None, count=None, overflow=None, pad=0):
    """One call on a chunk; the buffers are made (guard-filled, counters zero) unless given.  Returns the tensors."""
    from stnf import _native as N
    d = T.dev()
    nT, S = z.shape
    if scores is None:
        flat = torch.full((len(codes) * len(cols) * cap + pad,), GUARD, dtype=torch.float32, device=d)
        scores = (flat, flat[:len(codes) * len(cols) * cap].view(len(codes), len(cols), cap))
        count = torch.zeros(len(codes), dtype=torch.int64, device=d)
        overflow = torch.zeros(len(codes), dtype=torch.int32, device=d)
    ws = torch.empty(N.conformal_scores_workspace_bytes(S, nT) // 8, dtype=torch.float64, device=d)
    N.conformal_scores(torch.from_numpy(np.ascontiguousarray(y)).to(d), torch.from_numpy(np.ascontiguousarray(z)).to(d),
                       None if code is None else torch.from_numpy(np.ascontiguousarray(code)).to(d), cols, codes,
                       scores[1], count, overflow, ws)
    return scores, count, overflow


def run_select(keys, n, selections, n_max=None):
    """keys (C, stride) on the device, n a 1-element int64 tensor there; returns (value, rank_used) tensors."""
    from stnf import _native as N
    d = T.dev()
    k = len(selections)
    value = torch.full((k,), -3.0, dtype=torch.float32, device=d)
    used = torch.full((k,), -9, dtype=torch.int64, device=d)
    ws = torch.empty(N.select_workspace_bytes(k) // 8, dtype=torch.float64, device=d)
    N.select(keys, n, selections, value, used, ws, n_max=n_max)
    return value, used


def _n(n):
    return torch.tensor([n], dtype=torch.int64, device=T.dev())


# ------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("Q", cc.SCORE_Q)
def test_scores_are_numpy_bits_in_numpy_order_at_every_shape(Q):
    from stnf import calibration as CF
    cols = cc.score_cols(Q)
    runs = []
    for S in cc.SCORE_S:
        for nT in cc.SCORE_T:
            y, z, code = cc.make_score_case(S, nT, Q)
            ref = CF.scores_numpy(y, z, code, cols, cc.SEGMENT_CODES)
            cap = max(1, max(r.shape[1] for r in ref)) + 5
            runs.append((S, nT, ref, cap, run_scores(y, z, code, cols, cc.SEGMENT_CODES, cap)))
    for S, nT, ref, cap, ((_, scores), count, overflow) in runs:           # (the launches are queued before the reads)
        got, cnt = scores.cpu().numpy(), count.cpu().numpy()
        bad = cc.compare_segments(got, cnt, ref)
        assert not bad, (S, nT, Q, bad)
        assert not overflow.cpu().numpy().any()
        for g, r in enumerate(ref):                                        # nothing behind the members was written
            assert (got[g][:, r.shape[1]:] == GUARD).all(), (S, nT, Q, g)


def test_split_null_is_all_code_zero_and_one_segment():
    from stnf import calibration as CF
    y, z, _ = cc.make_score_case(257, 5, 3)
    cols = cc.score_cols(3)
    ref = CF.scores_numpy(y, z, None, cols, [0])
    (_, scores), count, _ = run_scores(y, z.reshape(1, -1), None, cols, [0], ref[0].shape[1])
    assert not cc.compare_segments(scores.cpu().numpy(), count.cpu().numpy(), ref)


@pytest.mark.parametrize("parts", [2, 3])
def test_a_grid_cut_into_calls_leaves_the_bytes_of_one_call(parts):
    S, nT, Q = 257, 17, 5
    y, z, code = cc.make_score_case(S, nT, Q, seed=2)
    cols = cc.score_cols(Q)
    cap = int(max(cc.conditions(y, z, code)["members"])) + 3
    (whole, _), wcount, _ = run_scores(y, z, code, cols, cc.SEGMENT_CODES, cap)
    cuts = [round(i * nT / parts) for i in range(parts + 1)]
    bufs = None
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        args = (y[t0 * S:t1 * S], z[t0:t1], code[t0:t1], cols, cc.SEGMENT_CODES, cap)
        bufs = run_scores(*args) if bufs is None else run_scores(*args, *bufs)
    (flat, _), count, overflow = bufs
    assert torch.equal(flat.view(torch.int32), whole.view(torch.int32)) and torch.equal(count, wcount)
    assert not overflow.any()


def test_a_capacity_below_the_member_count_sets_the_flag_and_keeps_the_prefix():
    from stnf import calibration as CF
    S, nT, Q = 513, 5, 3
    y, z, code = cc.make_score_case(S, nT, Q, seed=3)
    cols = cc.score_cols(Q)
    ref = CF.scores_numpy(y, z, code, cols, cc.SEGMENT_CODES)
    n0, n1 = (r.shape[1] for r in ref)
    cap = min(n0, n1) - 37
    assert cap > 64
    (flat, scores), count, overflow = run_scores(y, z, code, cols, cc.SEGMENT_CODES, cap, pad=4096)
    assert overflow.cpu().tolist() == [1, 1] and count.cpu().tolist() == [cap, cap]
    assert not cc.compare_segments(scores.cpu().numpy(), count.cpu().numpy(), ref, cap=cap)
    assert bool((flat[2 * len(cols) * cap:] == GUARD).all())               # the guard words behind the last segment
    # the smaller segment fits exactly, the larger does not: only its flag is set; the same chunk once more finds both
    # full, appends nothing and sets both flags
    assert n0 != n1
    cap, large = min(n0, n1), 0 if n0 > n1 else 1
    (flat, scores), count, overflow = run_scores(y, z, code, cols, cc.SEGMENT_CODES, cap, pad=64)
    assert overflow.cpu().tolist()[large] == 1 and overflow.cpu().tolist()[1 - large] == 0
    first = flat.clone()
    _, count, overflow = run_scores(y, z, code, cols, cc.SEGMENT_CODES, cap, (flat, scores), count, overflow)
    assert count.cpu().tolist() == [cap, cap] and overflow.cpu().tolist() == [1, 1]
    assert torch.equal(flat.view(torch.int32), first.view(torch.int32))
    assert not cc.compare_segments(scores.cpu().numpy(), count.cpu().numpy(), ref, cap=cap)
    assert bool((flat[2 * len(cols) * cap:] == GUARD).all())


# ------------------------------------------------------------------------------------------------ select
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_select_is_np_sort_by_value(family):
    d = T.dev()
    pending = []
    for n in cc.KEY_N:
        x = cc.make_keys(family, n)
        keys = torch.from_numpy(x).to(d).view(1, n)
        nd = _n(n)
        want = cc.ranks(n)
        for i in range(0, len(want), cc.MAX_SELECT):
            chunk = want[i:i + cc.MAX_SELECT]
            pending.append((x, chunk, run_select(keys, nd, [(0, r, None) for r in chunk])))
        # beyond n, and levels: k = ceil((n + 1) beta)
        betas = [0.0, 0.1, 0.5, 0.75, 0.9, 1.0]
        pending.append((x, [n, n + 5], run_select(keys, nd, [(0, n, None), (0, n + 5, None)])))
        pending.append((x, betas, run_select(keys, nd, [(0, None, b) for b in betas])))
    from stnf import calibration as CF
    ordered = {}
    for x, asked, (value, used) in pending:
        v, u = value.cpu().numpy(), used.cpu().numpy()
        if x.size not in ordered:
            ordered[x.size] = np.sort(x)
        for j, a in enumerate(asked):
            rank = a if isinstance(a, int) else CF.conformal_rank(x.size, a)
            if not isinstance(a, int) and rank < 0:
                rank = x.size                                              # a level beyond n: (+inf, -1)
            bad = cc.compare_select(x, rank, v[j], u[j], ordered[x.size])
            assert not bad, (family, x.size, a, bad)


def test_eight_columns_behind_a_stride_and_sixteen_selections():
    d = T.dev()
    n, stride, C = 65537, 65537 + 13, 8
    cols = [cc.make_keys(f, n, seed=1) for f in cc.FAMILIES[:C]]
    host = np.full((C, stride), np.float32(-77.0))                         # what lies behind n must not count
    for c, x in enumerate(cols):
        host[c, :n] = x
    keys = torch.from_numpy(host).to(d)
    sels = [(c, r, None) for c in range(C) for r in (0, n - 1)]            # 16, two per column
    sels[5] = (2, None, 0.5)
    sels[10] = (7, n // 2, None)
    sels[11] = (7, n // 3, None)                                           # four on column 7, none on column 5
    value, used = run_select(keys, _n(n), sels, n_max=n)
    again = run_select(keys, _n(n), sels, n_max=n)
    from stnf import calibration as CF
    v, u = value.cpu().numpy(), used.cpu().numpy()
    for j, (c, r, b) in enumerate(sels):
        rank = r if r is not None else CF.conformal_rank(n, b)
        assert not cc.compare_select(cols[c], rank, v[j], u[j]), (j, c, rank)
    assert torch.equal(value.view(torch.int32), again[0].view(torch.int32)) and torch.equal(used, again[1])
    # a device n below n_max: only the first n values count; a device n above it is read as n_max
    half = run_select(keys, _n(1000), [(0, 999, None), (0, 1000, None)], n_max=n)
    assert not cc.compare_select(cols[0][:1000], 999, half[0][0].item(), half[1][0].item())
    assert half[1][1].item() == -1 and np.isposinf(half[0][1].item())
    over = run_select(keys, _n(n + 100), [(0, n - 1, None), (0, n, None)], n_max=n)
    assert not cc.compare_select(cols[0], n - 1, over[0][0].item(), over[1][0].item()) and over[1][1].item() == -1


def test_n_comes_from_the_scores_calls_counter():
    """scores then select on one stream, no host read in between: the k-th smallest score of the calibration segment."""
    from stnf import calibration as CF
    S, nT, Q = 257, 17, 3
    y, z, code = cc.make_score_case(S, nT, Q, seed=4)
    cols = cc.score_cols(Q)
    ref = CF.scores_numpy(y, z, code, cols, cc.SEGMENT_CODES)
    cap = max(r.shape[1] for r in ref) + 9
    (_, scores), count, _ = run_scores(y, z, code, cols, cc.SEGMENT_CODES, cap)
    sels = [(c, None, 0.9) for c in range(len(cols))]
    for g in range(2):
        value, used = run_select(scores[g], count[g:g + 1], sels)
        for c in range(len(cols)):
            want = CF.select_level_numpy(ref[g][c], 0.9)
            assert value[c].item() == want[0] and used[c].item() == want[1], (g, c)


def test_select_under_graph_capture_replays_equal():
    from stnf import _native as N
    d = T.dev()
    n = 65537
    x = cc.make_keys("uniform", n, seed=2)
    keys = torch.from_numpy(x).to(d).view(1, n)
    nd = _n(n)
    sels = [(0, 0, None), (0, n // 2, None), (0, None, 0.9), (0, n - 1, None)]
    eager = run_select(keys, nd, sels)
    value = torch.zeros(len(sels), dtype=torch.float32, device=d)
    used = torch.zeros(len(sels), dtype=torch.int64, device=d)
    ws = torch.empty(N.select_workspace_bytes(len(sels)) // 8, dtype=torch.float64, device=d)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        N.select(keys, nd, sels, value, used, ws)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(value, eager[0]) and torch.equal(used, eager[1])
    # other data in the same buffers, another n in the same counter: the replay answers for what is there now
    x2 = cc.make_keys("seven", n, seed=3)
    keys.copy_(torch.from_numpy(x2).to(d).view(1, n))
    nd.fill_(n - 1000)
    graph.replay()
    torch.cuda.synchronize()
    from stnf import calibration as CF
    m = n - 1000
    for j, (c, r, b) in enumerate(sels):
        rank = r if r is not None else CF.conformal_rank(m, b)
        assert not cc.compare_select(x2[:m], rank, value[j].item(), used[j].item()), j


# ------------------------------------------------------------------------------------------------ end to end
def _field(d):
    coords, z, code = cc.e2e_field()
    tv = cc.grid_times(cc.E2E_T)
    return coords, z, code, tuple(torch.from_numpy(a).to(d) for a in (coords, tv, z, code))


def _restated(grid, z, code, levels, intervals, alpha, cal=2, ev=3):
    from stnf import calibration as CF
    plan = CF.make_plan(grid.shape[-1], levels, intervals, alpha)
    return plan, CF.finish_host(plan, CF.scores_numpy(grid, z, code, plan.cols, [cal, ev]))


def _same_report(got, plan, fin):
    from stnf import calibration as CF
    want = CF.report(plan, fin)
    assert got["n_cal"] == want["n_cal"] and got["n_eval"] == want["n_eval"] and got["overflow"] == [False, False]
    assert got["rank_beyond_n"] == want["rank_beyond_n"]
    if "levels" in want:
        for key in ("offset", "rank_used", "reliability_before", "reliability_after"):
            assert np.array_equal(got["levels"][key], want["levels"][key]), key           # equal, not merely close
        for a, b in zip(got["intervals"], want["intervals"]):
            for key in ("offset", "rank_used", "n_cal", "coverage_before", "coverage_after"):
                assert a[key] == b[key], key
            # the two widths are float64 sums of the same float32 scores in another order
            assert abs(a["mean_width_before"] - b["mean_width_before"]) <= 1e-12 * max(1.0, abs(b["mean_width_before"]))
            assert a["mean_width_after"] == a["mean_width_before"] + 2.0 * a["offset"]
    else:
        assert got["abs"] == want["abs"]


def test_conformal_grid_equals_the_restatement_of_predict_grid():
    from stnf.engine import Predictor
    d = T.dev()
    m = cc.e2e_model().to(d)
    coords, z, code, (ct, tvt, zt, codet) = _field(d)
    pr = Predictor(m)
    grid = pr.predict_grid(ct, tvt, max_rows=cc.E2E_MAX_ROWS).cpu().numpy()
    plan, fin = _restated(grid, z, code, cc.E2E_LEVELS, [cc.E2E_INTERVAL], cc.E2E_ALPHA)
    assert fin["count"].min() > 60 and (fin["rank_used"] >= 0).all()
    for max_rows, cap in ((cc.E2E_MAX_ROWS, int(fin["count"].max())), (None, None)):
        got = pr.conformal_grid(ct, tvt, zt, codet, cc.E2E_LEVELS, [cc.E2E_INTERVAL], cc.E2E_ALPHA, max_rows=max_rows,
                                cap=cap)
        _same_report(got, plan, fin)
        assert np.array_equal(got["calibration"].interval_offsets, fin["value"][3:])
    # too few calibration entries for the level: reported as +inf and -1
    got = pr.conformal_grid(ct, tvt, zt, codet, cc.E2E_LEVELS, [cc.E2E_INTERVAL], 1e-4, max_rows=cc.E2E_MAX_ROWS)
    assert got["rank_beyond_n"] and np.isposinf(got["intervals"][0]["offset"]) and got["intervals"][0]["rank_used"] == -1
    # a capacity below the members: the flag comes back
    got = pr.conformal_grid(ct, tvt, zt, codet, cc.E2E_LEVELS, None, cc.E2E_ALPHA, cap=40)
    assert got["overflow"] == [True, True] and got["n_cal"] == 40
    # a mean model: the half-width of |z - yhat|
    mm = cc.e2e_model(quantiles=False).to(d)
    pm = Predictor(mm)
    grid = pm.predict_grid(ct, tvt).cpu().numpy()
    plan, fin = _restated(grid, z, code, None, None, 0.1)
    _same_report(pm.conformal_grid(ct, tvt, zt, codet, alpha=0.1, max_rows=cc.E2E_MAX_ROWS), plan, fin)


def test_grid_scores_with_and_without_the_key():
    from stnf.engine import Predictor
    from stnf.utils import grid_scores
    d = T.dev()
    m = cc.e2e_model().to(d)
    coords, z, code, (ct, tvt, _, _) = _field(d)
    config = {"regression_type": "multi-quantile", "quantile_levels": cc.E2E_LEVELS, "interval": cc.E2E_INTERVAL,
              "quantile_diagnostics": True}
    masks = [code == c for c in (1, 2, 3)]
    plain = grid_scores(m, z, coords, *masks, config=config, max_rows=cc.E2E_MAX_ROWS)
    got = grid_scores(m, z, coords, *masks, config=dict(config, conformal=True), max_rows=cc.E2E_MAX_ROWS)
    assert "conformal" not in plain and set(got) == set(plain) | {"conformal"}
    for name in plain["splits"]:
        assert plain["splits"][name] == got["splits"][name], name
        for k, v in plain["quantile"][name].items():
            assert np.array_equal(np.asarray(v), np.asarray(got["quantile"][name][k]), equal_nan=True), (name, k)
    for k in ("site_mse", "time_mse", "site_count"):
        assert np.array_equal(plain[k], got[k], equal_nan=True)
    grid = Predictor(m).predict_grid(ct, tvt).cpu().numpy()
    plan, fin = _restated(grid, z, code, cc.E2E_LEVELS, [cc.E2E_INTERVAL], cc.E2E_ALPHA)
    cf = got["conformal"]
    assert cf["alpha"] == cc.E2E_ALPHA and cf["split"] == "valid"
    _same_report(cf, plan, fin)
    iv = cf["intervals"][0]
    assert iv["coverage_before"] == got["splits"]["test"]["coverage"] == got["quantile"]["test"]["coverage"]
    assert abs(iv["mean_width_before"] - got["splits"]["test"]["mean_width"]) <= 1e-6
    assert np.array_equal(cf["levels"]["reliability_before"], got["quantile"]["test"]["reliability"])


def test_apply_then_the_quantile_diagnostics_show_the_reported_coverage():
    """The calibrated interval, scored by stdadk_quantile_diag_f32: INSIDE / N of the test split is the coverage the
    calibration reported from the scores, and BELOW / N of every shifted level its reliability after."""
    from stnf import _native as N
    from stnf.engine import Predictor
    d = T.dev()
    m = cc.e2e_model().to(d)
    coords, z, code, (ct, tvt, zt, codet) = _field(d)
    pr = Predictor(m)
    got = pr.conformal_grid(ct, tvt, zt, codet, cc.E2E_LEVELS, [cc.E2E_INTERVAL], cc.E2E_ALPHA, max_rows=cc.E2E_MAX_ROWS)
    record = got["calibration"]
    grid = pr.predict_grid(ct, tvt)
    S, Tn, Q = cc.E2E_S, cc.E2E_T, len(cc.E2E_LEVELS)
    ws = torch.empty(N.quantile_diag_workspace_bytes(S, Tn) // 8, dtype=torch.float64, device=d)

    def diag(pred):
        acc = torch.zeros(4, N.QD_SLOTS, dtype=torch.float64, device=d)
        N.quantile_diag(pred.reshape(Tn * S, Q).contiguous(), zt, codet, cc.E2E_LEVELS, 0, Q - 1, acc, None, None, ws)
        return acc.cpu().numpy()[3]
    before, wide, shifted = diag(grid), diag(record.apply(grid, cc.E2E_INTERVAL)), diag(record.apply(grid))
    iv = got["intervals"][0]
    assert before[N.QD_N] == got["n_eval"] and before[N.QD_INSIDE] / before[N.QD_N] == iv["coverage_before"]
    assert wide[N.QD_INSIDE] / wide[N.QD_N] == iv["coverage_after"] > iv["coverage_before"]
    assert np.array_equal(shifted[N.QD_BELOW:N.QD_BELOW + Q] / shifted[N.QD_N], got["levels"]["reliability_after"])


@pytest.mark.parametrize("n", [1, 300, 65536 + 300])
def test_evaluator_and_evaluate_model_calibrate_a_validation_set(n):
    from stnf import calibration as CF
    from stnf.dataio import DeviceDataset
    from stnf.evaluation import Evaluator
    from stnf.utils.predictions import evaluate_model
    d = T.dev()
    rs = np.random.RandomState(50 + n % 7)
    coords, t = rs.uniform(0, 1, (n, 2)).astype(np.float32), rs.uniform(0, 1, (n, 1)).astype(np.float32)
    y = (0.3 * rs.standard_normal((n, 1))).astype(np.float32)
    ds = DeviceDataset(*(torch.from_numpy(a).to(d) for a in (coords, t, y)))
    m = cc.e2e_model().to(d)
    ev = Evaluator(m, loss="pinball", quantile_levels=cc.E2E_LEVELS, max_batch=65536)
    plain = ev.evaluate(ds, 65536)
    sums = list(ev.sums)
    got = ev.evaluate(ds, 65536, conformal=cc.E2E_ALPHA)
    assert ev.sums == sums and {k: v for k, v in got.items() if k != "calibration"} == plain
    pred = ev.predictions.cpu().numpy()
    want = CF.calibrate_rows(pred, y.reshape(-1), cc.E2E_LEVELS, [cc.E2E_INTERVAL], cc.E2E_ALPHA)      # the host path
    for rec in (got["calibration"], evaluate_model(m, ds, {"regression_type": "multi-quantile",
                                                           "quantile_levels": cc.E2E_LEVELS, "conformal": True,
                                                           "interval": cc.E2E_INTERVAL})["calibration"]):
        assert rec.n_cal == n and rec.alpha == cc.E2E_ALPHA
        assert np.array_equal(rec.level_offsets, want.level_offsets) and np.array_equal(rec.rank_used, want.rank_used)
        assert np.array_equal(rec.interval_offsets, want.interval_offsets)
    if n == 1:
        assert (want.rank_used == [0, 0, -1, -1]).all() and np.isposinf(want.interval_offsets[0])
    # a mean model: |y - yhat|
    mm = cc.e2e_model(quantiles=False).to(d)
    em = Evaluator(mm, max_batch=65536)
    rec = em.evaluate(ds, 65536, conformal=0.1)["calibration"]
    want = CF.calibrate_rows(em.predictions.cpu().numpy(), y.reshape(-1), alpha=0.1)
    assert rec.abs_offset == want.abs_offset and np.array_equal(rec.rank_used, want.rank_used) and len(rec.levels) == 0
