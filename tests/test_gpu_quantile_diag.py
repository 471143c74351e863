"""Quantile diagnostics on the device: stdadk_quantile_diag_f32 through the ABI on the generated cases of
tests/golden/quantile_diag_cases.py against its float64 restatement -- every count EXACT, every float sum within the
derived bound (n + 3) 2^-53 sum|term|, every slot compared -- at the shapes named from the kernel's constants; chunked
calls, repeated calls, accumulation; then end to end: Predictor.quantile_grid and score_grid(quantile=True) on the
window, materialising and expanded routes against the restatement of predict_grid's own output, grid_scores' `quantile`
entry, and Evaluator.evaluate(diagnostics=True) on a pinball model and a delta-head model."""
import numpy as np
import pytest
import torch

from golden import quantile_diag_cases as qc
import test_gpu_parity as T

pytestmark = pytest.mark.gpu


def run_kernel(y, z, code, taus, lo, hi, site=True, time=True, accs=None):
    """The call on zeroed accumulators (time_acc pre-filled: it is assigned, not added to), or on `accs`."""
    from stnf import _native as N
    d = T.dev()
    nT, S = z.shape
    if accs is None:
        accs = (torch.zeros(4, N.QD_SLOTS, dtype=torch.float64, device=d),
                torch.zeros(4, S, 4, dtype=torch.float64, device=d) if site else None,
                torch.full((4, nT, 4), -7.0, dtype=torch.float64, device=d) if time else None)
    ws = torch.empty(N.quantile_diag_workspace_bytes(S, nT) // 8, dtype=torch.float64, device=d)
    N.quantile_diag(torch.from_numpy(y).to(d), torch.from_numpy(z).to(d),
                    None if code is None else torch.from_numpy(code).to(d),
                    None if taus is None else [float(t) for t in taus], lo, hi, *accs, ws)
    return accs


def host(accs):
    return [None if a is None else a.cpu().numpy() for a in accs]


@pytest.mark.parametrize("Q", range(1, qc.MAX_Q + 1))
def test_kernel_matches_restatement_at_every_shape(Q):
    """S in {1, 63, 64, 65, W-1, W, W+1, 2W+1} x nT in {1, U-1, U, U+1, TT-1, TT, TT+1, 2TT+1} for this Q; interval on
    and off, split NULL and given, site_acc and time_acc NULL and given run through all sixteen combinations along S,
    along nT and along Q (quantile_diag_cases.toggles)."""
    from stnf import _native as N
    assert (N.QD_N, N.QD_BELOW, N.QD_PIT, N.QD_CROSS_ROWS, N.QD_PAIR, N.QD_DEPTH1, N.QD_DEPTH2, N.QD_CRPS, N.QD_INSIDE,
            N.QD_SLOTS) == (qc.N_, qc.BELOW, qc.PIT, qc.CROSS_ROWS, qc.PAIR, qc.DEPTH1, qc.DEPTH2, qc.CRPS, qc.INSIDE,
                            qc.SLOTS)
    sizes, slices = qc.kernel_shapes(Q)
    taus = qc.levels(Q)
    seen = set()
    runs = []
    for i_s, S in enumerate(sizes):
        for i_t, nT in enumerate(slices):
            interval, with_split, with_site, with_time = tog = qc.toggles(i_s, i_t, Q)
            seen.add(tog)
            y, z, code = qc.make_case(S, nT, Q)
            lo, hi = (0, Q - 1) if interval else (-1, -1)
            code = code if with_split else None
            runs.append((S, nT, tog, y, z, code, lo, hi, run_kernel(y, z, code, taus, lo, hi, with_site, with_time)))
    assert len(seen) == (16 if Q >= 2 else 8)
    worst = 0.0
    for S, nT, tog, y, z, code, lo, hi, accs in runs:                  # (the launches are all queued before the reads)
        got = host(accs)
        ref = qc.restate(y, z, code, taus, lo, hi)
        bound = qc.bounds(y, z, code, taus, lo, hi)
        bad = qc.compare(got, ref, bound)
        assert not bad, (S, nT, Q, tog, bad[:5])
        assert got[0][:, qc.N_].sum() == (np.isfinite(z) & (True if code is None else code < 4)).sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.abs(got[0][:, qc.CRPS] - ref[0][:, qc.CRPS]) / bound[0][:, qc.CRPS]
        worst = max(worst, float(np.nanmax(np.where(np.isfinite(r), r, 0.0))))
    print(f"Q={Q}: {len(runs)} shapes, worst |delta CRPS| / bound = {worst:.3f}")


def test_chunks_of_1_3_and_all_slices_give_the_same_bits():
    """A grid cut into chunks of 1, 3 and all its slices: site_acc bit-identical, every count identical, the float split
    sums within the bound, and each chunk's time_acc equal to the whole call's rows."""
    S, nT, Q = 2 * qc.SITES_PER_WG + 1, 2 * qc.TILE_SLICES + 1, 5
    y, z, code = qc.make_case(S, nT, Q, seed=3)
    taus = qc.levels(Q)
    whole = host(run_kernel(y, z, code, taus, 0, Q - 1))
    ref = qc.restate(y, z, code, taus, 0, Q - 1)
    bound = qc.bounds(y, z, code, taus, 0, Q - 1)
    assert not qc.compare(whole, ref, bound)
    from stnf import _native as N
    d = T.dev()
    for per in (1, 3):
        accs = (torch.zeros(4, N.QD_SLOTS, dtype=torch.float64, device=d),
                torch.zeros(4, S, 4, dtype=torch.float64, device=d))
        times = []
        for t0 in range(0, nT, per):
            n = min(per, nT - t0)
            tacc = torch.full((4, n, 4), -7.0, dtype=torch.float64, device=d)
            run_kernel(y[t0 * S:(t0 + n) * S], z[t0:t0 + n], code[t0:t0 + n], taus, 0, Q - 1, accs=accs + (tacc,))
            times.append(tacc)
        split, site = host(accs)
        tall = torch.cat(times, dim=1).cpu().numpy()
        assert np.array_equal(site, whole[1]), per
        assert np.array_equal(tall, whole[2]), per
        assert np.array_equal(split[:, qc.COUNT_SLOTS], whole[0][:, qc.COUNT_SLOTS]), per
        assert not qc.compare((split, site, tall), ref, bound), per


def test_same_call_same_bits():
    S, nT, Q = 2 * qc.SITES_PER_WG + 1, qc.TILE_SLICES + 1, 8
    y, z, code = qc.make_case(S, nT, Q, seed=4)
    a = host(run_kernel(y, z, code, qc.levels(Q), 1, 6))
    b = host(run_kernel(y, z, code, qc.levels(Q), 1, 6))
    for x, w in zip(a, b):
        assert np.array_equal(x, w)


def test_accumulates_onto_what_is_there():
    """split_acc and site_acc are ADDED to (every slot the call does not use keeps its value), time_acc is assigned.  The
    value already there is one more term of each float sum (quantile_diag_cases.bounds, `start`)."""
    from stnf import _native as N
    S, nT, Q = qc.SITES_PER_WG + 1, 5, 3
    y, z, code = qc.make_case(S, nT, Q, seed=5)
    taus = qc.levels(Q)
    rs = np.random.RandomState(6)
    start = (rs.randint(0, 50, size=(4, N.QD_SLOTS)).astype(np.float64), rs.randint(0, 50, size=(4, S, 4)).astype(np.float64))
    start[0][:, qc.FLOAT_SLOTS] += rs.uniform(size=(4, 3))
    start[1][:, :, qc.SV_CRPS] += rs.uniform(size=(4, S))
    d = T.dev()
    accs = (torch.from_numpy(start[0]).to(d), torch.from_numpy(start[1]).to(d),
            torch.full((4, nT, 4), -7.0, dtype=torch.float64, device=d))
    got = host(run_kernel(y, z, code, taus, 0, 2, accs=accs))
    ref = qc.restate(y, z, code, taus, 0, 2)
    bad = qc.compare(got, ref, qc.bounds(y, z, code, taus, 0, 2, start=start), start=start)
    assert not bad, bad[:5]


@pytest.mark.parametrize("case,word", [("Q", "Q=9"), ("lo_ge_hi", "interval"), ("workspace", "workspace")])
def test_kernel_refuses_bad_arguments(case, word):
    from stnf import _native as N
    S, nT, Q = 67, 3, 9 if case == "Q" else 5
    d = T.dev()
    accs = (torch.full((4, N.QD_SLOTS), 3.0, dtype=torch.float64, device=d),
            torch.full((4, S, 4), 3.0, dtype=torch.float64, device=d),
            torch.full((4, nT, 4), 3.0, dtype=torch.float64, device=d))
    ws = torch.empty(N.quantile_diag_workspace_bytes(S, nT) // 8, dtype=torch.float64, device=d)
    with pytest.raises(RuntimeError, match=word):
        N.quantile_diag(torch.zeros(nT * S, Q, device=d), torch.zeros(nT, S, device=d), None, None,
                        3 if case == "lo_ge_hi" else 0, 3, *accs, ws[:-1] if case == "workspace" else ws)
    torch.cuda.synchronize()
    assert all(bool((a == 3.0).all()) for a in accs)           # nothing was launched


# ------------------------------------------------------------------------------------------------ end to end
def _field(d):
    coords, z, code = qc.e2e_field()
    tv = qc.grid_times(qc.E2E_T)
    return coords, z, code, tuple(torch.from_numpy(a).to(d) for a in (coords, tv, z, code))


@pytest.mark.parametrize("route", list(qc.ROUTES))
def test_quantile_grid_equals_restatement_of_predict_grid(route):
    """quantile_grid and score_grid(quantile=True), one chunk and chunks of 3 slices (max_rows cutting the grid), against
    the restatement applied to the device's own predict_grid output read back: counts exact, sums within the bound.
    The CRPS slot agrees with 2/Q x the sum of the CHECK slots of stdadk_grid_score_f32 within the same bound;
    score_grid without the flag returns what it did, bit for bit."""
    from stnf import _native as N
    from stnf.engine import Predictor
    d = T.dev()
    spec = qc.ROUTES[route]
    m = qc.e2e_model(hidden=spec["hidden"])
    m.force_window_path = spec["force_window"]
    m = m.to(d)
    Q, S, Tn = m.output_dim, qc.E2E_S, qc.E2E_T
    coords, z, code, (ct, tvt, zt, codet) = _field(d)
    taus32 = np.asarray(qc.E2E_LEVELS, dtype=np.float32)
    lo, hi = 0, Q - 1
    pr = Predictor(m, chunk=4096)
    parts = bool(pr.state.flags & N.FLAG_W0_T) and N.forward_parts_supported(pr.state.desc)
    assert parts == (route != "expanded")
    assert N.step_uses_window(pr.state.basis, pr.state.desc, pr.state.flags) == (route == "window")
    for max_rows in (None, 3 * S + 5):
        grid = pr.predict_grid(ct, tvt, max_rows=max_rows).cpu().numpy()
        ref = qc.restate(grid, z, code, taus32, lo, hi)
        bound = qc.bounds(grid, z, code, taus32, lo, hi)
        if route == "materialising":                  # the model the CPU test looks at: crossing and sorted rows
            assert (ref[0][:, qc.CROSS_ROWS] > 0).all() and (ref[0][:, qc.CROSS_ROWS] < ref[0][:, qc.N_]).all()
        kw = dict(split=codet, quantile_levels=qc.E2E_LEVELS, interval=qc.E2E_INTERVAL, max_rows=max_rows)
        got = host(pr.quantile_grid(ct, tvt, zt, **kw))
        assert [g.shape for g in got] == [(4, N.QD_SLOTS), (4, S, 4), (4, Tn, 4)]
        bad = qc.compare(got, ref, bound)
        assert not bad, (route, max_rows, bad[:5])
        plain = [a.clone() for a in pr.score_grid(ct, tvt, zt, **kw)]
        both = pr.score_grid(ct, tvt, zt, quantile=True, **kw)
        assert len(plain) == 3 and len(both) == 6
        for a, b in zip(plain, both[:3]):
            assert torch.equal(a, b)
        for a, b in zip(got, host(both[3:])):
            assert np.array_equal(a, b)
        check = plain[0][:, N.GRID_CHECK:N.GRID_CHECK + Q].cpu().numpy().sum(axis=1) * (2.0 / Q)
        delta = np.abs(check - got[0][:, qc.CRPS])
        print(f"{route} max_rows={max_rows}: |CRPS - 2/Q sum CHECK| = {delta.tolist()}, bound {bound[0][:, qc.CRPS].tolist()}")
        assert (delta <= bound[0][:, qc.CRPS]).all()


def test_grid_scores_quantile_entry():
    """grid_scores with `quantile_diagnostics`: the per-split entries and the maps are the restatement's sums of the
    device's own grid, divided; without the key the dict has no `quantile` entry."""
    from stnf.engine import Predictor
    from stnf.utils import grid_scores
    d = T.dev()
    m = qc.e2e_model().to(d)
    coords, z, code, (ct, tvt, _, _) = _field(d)
    Q = m.output_dim
    config = {"regression_type": "multi-quantile", "quantile_levels": qc.E2E_LEVELS, "interval": qc.E2E_INTERVAL}
    masks = [code == c for c in (1, 2, 3)]
    plain = grid_scores(m, z, coords, *masks, config=config, max_rows=3 * qc.E2E_S + 5)
    assert "quantile" not in plain
    got = grid_scores(m, z, coords, *masks, config=dict(config, quantile_diagnostics=True), max_rows=3 * qc.E2E_S + 5)
    assert set(got) == set(plain) | {"quantile"}
    for k in plain["splits"]["all"]:
        assert plain["splits"]["all"][k] == got["splits"]["all"][k], k
    grid = Predictor(m).predict_grid(ct, tvt).cpu().numpy()
    taus32 = np.asarray(qc.E2E_LEVELS, dtype=np.float32)
    split, site, time = qc.restate(grid, z, code, taus32, 0, Q - 1)
    bsplit, bsite, btime = qc.bounds(grid, z, code, taus32, 0, Q - 1)
    qd = got["quantile"]
    for name, c in (("other", 0), ("train", 1), ("valid", 2), ("test", 3)):
        e, n = qd[name], split[c, qc.N_]
        assert e["rows"] == n > 0
        assert np.array_equal(e["reliability"], split[c, qc.BELOW:qc.BELOW + Q] / n)
        assert np.array_equal(e["pit"], split[c, qc.PIT:qc.PIT + Q + 1] / n) and abs(e["pit"].sum() - 1) < 1e-12
        assert e["cross_rate"] == split[c, qc.CROSS_ROWS] / n and e["coverage"] == split[c, qc.INSIDE] / n
        assert np.array_equal(e["pair_cross_rate"], split[c, qc.PAIR:qc.PAIR + Q - 1] / n)
        for key, slot in (("nc_penalty_p1", qc.DEPTH1), ("nc_penalty_p2", qc.DEPTH2), ("crps", qc.CRPS)):
            assert abs(e[key] * n - split[c, slot]) <= bsplit[c, slot] + 2.0 ** -52 * abs(split[c, slot]), (name, key)
    assert qd["all"]["rows"] == split[:, qc.N_].sum()
    assert np.array_equal(qd["site_count"], site[:, :, qc.SV_N].sum(axis=0))
    assert np.array_equal(qd["time_count"], time[:, :, qc.SV_N].sum(axis=0))
    assert np.array_equal(qd["site_cross_rate"], site[:, :, qc.SV_CROSS].sum(axis=0) / site[:, :, qc.SV_N].sum(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = site[:, :, qc.SV_CRPS] / site[:, :, qc.SV_N]
        tol = (bsite + 2.0 ** -52 * np.abs(site[:, :, qc.SV_CRPS])) / site[:, :, qc.SV_N]
    ok = site[:, :, qc.SV_N] > 0
    assert np.array_equal(np.isnan(qd["site_crps_by_split"]), ~ok)
    assert (np.abs(qd["site_crps_by_split"] - ref)[ok] <= tol[ok]).all()
    assert qd["time_crps_by_split"].shape == (4, qc.E2E_T) and qd["site_coverage"].shape == (qc.E2E_S,)


def _dataset(n, d, seed):
    from stnf.dataio import DeviceDataset
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (n, 2)).astype(np.float32)
    t = rs.uniform(0, 1, (n, 1)).astype(np.float32)
    y = (0.3 * rs.standard_normal((n, 1))).astype(np.float32)
    return DeviceDataset(*(torch.from_numpy(a).to(d) for a in (coords, t, y))), y


@pytest.mark.parametrize("head", ["pinball_nc", "delta"])
@pytest.mark.parametrize("n", [1, 300, 65536 + 300])
def test_evaluator_diagnostics(head, n):
    """Evaluator.evaluate(diagnostics=True) on 1, 300 and 65 536 + 300 rows (a ragged last batch): the `quantile` entry
    is the restatement of the returned predictions; the delta head's quantiles never cross (cross_rate and both
    penalties exactly 0); with diagnostics=False the dict and self.sums are what they are without the feature."""
    from stnf.evaluation import Evaluator
    d = T.dev()
    delta = head == "delta"
    m = qc.e2e_model(delta=delta).to(d)
    Q = m.output_dim
    kw = dict(non_crossing_lambda=0.1) if delta else dict(non_crossing_weight=0.5, non_crossing_power=2)
    ev = Evaluator(m, loss="pinball", quantile_levels=qc.E2E_LEVELS, max_batch=65536, **kw)
    ds, y = _dataset(n, d, 40 + n % 7)
    plain = ev.evaluate(ds, 65536)
    sums = list(ev.sums)
    assert "quantile" not in plain and ev.quantile_sums is None and ev.predictions is None
    got = ev.evaluate(ds, 65536, diagnostics=True)
    assert ev.sums == sums and {k: v for k, v in got.items() if k != "quantile"} == plain
    pred = ev.predictions.cpu().numpy()
    assert pred.shape == (n, Q)
    taus32 = np.asarray(qc.E2E_LEVELS, dtype=np.float32)
    z = y.reshape(1, n)
    ref = qc.restate(pred, z, None, taus32)
    bound = qc.bounds(pred, z, None, taus32)
    acc = np.zeros((4, qc.SLOTS))
    acc[0] = ev.quantile_sums
    bad = qc.compare((acc, None, None), ref, bound)
    assert not bad, bad[:5]
    e, row = got["quantile"], ref[0][0]
    assert e["rows"] == n and np.array_equal(e["reliability"], row[qc.BELOW:qc.BELOW + Q] / n)
    assert np.array_equal(e["pit"], row[qc.PIT:qc.PIT + Q + 1] / n) and e["cross_rate"] == row[qc.CROSS_ROWS] / n
    assert "coverage" not in e and list(e["levels"]) == qc.E2E_LEVELS
    # the check-loss slots of the first accumulator are the same products in another order
    crps_eval = got["crps"]
    assert abs(e["crps"] - crps_eval) <= 1e-5 * abs(crps_eval)          # (those are float32 element terms)
    if delta:
        assert e["cross_rate"] == 0.0 and e["nc_penalty_p1"] == 0.0 and e["nc_penalty_p2"] == 0.0
        assert not e["pair_cross_rate"].any()
    elif n > 1:
        assert 0.0 < e["cross_rate"] and e["nc_penalty_p1"] > 0.0 and e["nc_penalty_p2"] > 0.0
