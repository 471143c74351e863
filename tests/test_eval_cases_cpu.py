"""CPU half of the per-batch validation tests (the GPU half: test_gpu_eval_batches.py): the teeth of the comparator.

A float32 numpy emulation of csrc/eval.hip's order of operations -- per-thread sequential float sums in the kernel's
row order with its Q objective terms per row, a 64-lane tree in float, the four wave sums of a workgroup added in
double, the partials added in double by 256 striding threads and a tree -- is
  (a) inside the reduction bound of golden/eval_cases.py for every slot, batch size and head of the table: the one thing
      that justifies the formula;
  (b) outside it for each mutant of the pass, at the sizes where the mutant applies;
and (c) the table's own edge assertions hold.
"""
import numpy as np
import pytest

from golden import eval_cases as ec

F32 = np.float32


def _fma(a, b, c):
    """float32 fma(a, b, c): the product of two floats is exact in double"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _element_terms(yp, y, head, metric_col):
    """float32 element terms as the kernel's row body and csrc/loss.h form them: (dm, obj (B, Q), check (B, Q))"""
    B, Q = yp.shape
    yt = np.ascontiguousarray(np.broadcast_to(y, (B, Q))) if y.shape[1] == 1 else y
    dm = yp[:, metric_col] - yt[:, metric_col]
    tau = ec.head_taus(head)[None, :]
    e = yt - yp
    check = np.maximum((tau - F32(1.0)) * e, tau * e)
    if head["kind"] == "pinball":
        obj = check.copy()
        if head["nc_weight"] > 0 and Q > 1:
            d = yp[:, :-1] - yp[:, 1:]
            f = np.where(d > 0, d if head["nc_power"] == 1 else d * d, F32(0.0)).astype(F32)
            w = np.full_like(f, F32(head["nc_weight"]) * F32(Q))
            obj[:, :-1] = _fma(w, f, obj[:, :-1])
    else:
        d = yp - yt
        obj = d * d
    assert dm.dtype == obj.dtype == check.dtype == F32
    return dm, obj, check


def _strided(term, B, trips):
    """(trips, stride): row r of trip k is the row thread r reads on its k-th pass; 0 beyond the batch (x + 0 is exact)"""
    s = ec.stride(B)
    out = np.zeros(trips * s, F32)
    out[:len(term)] = term
    return out.reshape(trips, s)


def _wave_tree(v):
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    assert v.dtype == F32
    return v[..., 0]


def _finish(parts):
    """eval_finish_kernel for one value: thread i adds partials i, i + 256, ... in order, then a tree, in double"""
    n = len(parts)
    pad = np.zeros(-(-n // ec.EVAL_T) * ec.EVAL_T)
    pad[:n] = parts
    s = np.zeros(ec.EVAL_T)
    for chunk in pad.reshape(-1, ec.EVAL_T):
        s = s + chunk
    o = ec.EVAL_T // 2
    while o > 0:
        s = s[:o] + s[o:2 * o]
        o //= 2
    return float(s[0])


def emulate(yp, y, head, batch_weight, start=None, rows=None, max_trips=None, max_partials=None, metric_col=None,
            weight_sse=False, stray_check=False):
    """The accumulator after one call that started from `start` (zeros).  The keyword arguments are the mutants:
    `rows` (the kernel believes the batch has that many), `max_trips`, `max_partials`, another `metric_col`, the batch
    weight on SSE too, a check-loss slot written at index Q."""
    yp, y = np.asarray(yp, F32), np.asarray(y, F32)
    B, Q = yp.shape
    n = B if rows is None else rows
    dm, obj, check = _element_terms(yp[:n], y[:n], head, head["metric_col"] if metric_col is None else metric_col)
    nblk, trips = ec.partials_blocks(B), ec.rows_per_thread(B)
    run = trips if max_trips is None else min(trips, max_trips)
    dms = _strided(dm, B, trips)
    objs = [_strided(obj[:, q], B, trips) for q in range(Q)]
    chks = [_strided(check[:, q], B, trips) for q in range(Q)]
    zero = np.zeros(ec.stride(B), F32)
    acc = {"objective": zero, "sse": zero, "sae": zero, **{f"check{q}": zero for q in range(Q)}}
    for k in range(run):
        acc["sse"] = _fma(dms[k], dms[k], acc["sse"])
        acc["sae"] = acc["sae"] + np.abs(dms[k])
        for q in range(Q):
            acc["objective"] = acc["objective"] + objs[q][k]
            acc[f"check{q}"] = acc[f"check{q}"] + chks[q][k]
    out = np.zeros(ec.EVAL_SLOTS) if start is None else np.array(start, np.float64)
    slots = {"objective": ec.EVAL_OBJECTIVE, "sse": ec.EVAL_SSE, "sae": ec.EVAL_SAE,
             **{f"check{q}": ec.EVAL_CHECK + q for q in range(Q)}}
    for name, v in acc.items():
        waves = _wave_tree(v.reshape(nblk, ec.EVAL_T // ec.WAVE, ec.WAVE)).astype(np.float64)
        parts = (waves[:, 0] + waves[:, 1]) + (waves[:, 2] + waves[:, 3])
        total = _finish(parts if max_partials is None else parts[:max_partials])
        if name == "objective" or (name == "sse" and weight_sse):
            total *= batch_weight
        out[slots[name]] += total
    if stray_check and Q < ec.MAX_Q:
        out[ec.EVAL_CHECK + Q] += out[ec.EVAL_CHECK + Q - 1]
    out[ec.EVAL_ROWS] += n
    out[ec.EVAL_BATCHES] += 1.0
    return out


def _case(B, head, kind="arange", seed=5):
    """(rows, yp, y): make_rows of the head, synthetic float32 predictions in the caller's order, the targets at idx
    with the ties set from those predictions -- what the GPU test does with the predictions the pass returns."""
    Q = head["Q"]
    rows = ec.make_rows(B, Q, head["y_cols"], seed + B % 1000, kind)
    rs = np.random.RandomState(B % 9973 + 31 * Q)
    yp = (0.7 * rs.standard_normal((B, Q)) + 0.1 * np.arange(Q)[None, :]).astype(F32)
    ec.set_ties(rows["y"], rows["idx"], yp, rows["ties"])
    return rows, yp, rows["y"][rows["idx"]]


def _judge(got, yp, y, head, w, start=None):
    add, _, bound = ec.reference(yp, y, head, w)
    return ec.compare_accumulator(got, np.zeros(ec.EVAL_SLOTS) if start is None else start, add, bound, head["Q"])


def test_table_edges():
    ec.check_table()
    assert [ec.partials_blocks(b) for b in (0, 1, 256, 257, 262144, 262145, 2 ** 31 - 1)] == [1, 1, 1, 2, 1024, 1024, 1024]
    assert [ec.rows_per_thread(b) for b in (1, 262144, 262145, 524288, 524289, 1048576)] == [1, 1, 2, 2, 3, 4]
    for B in ec.BATCH_SIZES:
        for kind in ec.INDEX_KINDS:
            if B > 1023 and kind != "arange":
                continue
            idx = ec.make_index(kind, B, 3)
            assert idx.shape == (B,) and idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < ec.resident_rows(kind, B)
    B = 1023
    assert np.array_equal(np.sort(ec.make_index("permutation", B, 3)), np.arange(B))
    assert not np.array_equal(ec.make_index("permutation", B, 3), np.arange(B))
    sub = ec.make_index("subset", B, 3)
    assert len(set(sub.tolist())) == B < ec.resident_rows("subset", B) and sub.max() >= B
    assert len(set(ec.make_index("all_same", B, 3).tolist())) == 1
    assert len(set(ec.make_index("few_repeated", B, 3).tolist())) == 7


# the heads a planted row feeds least: the extreme levels of Q = 8 under broadcast and column targets with the power-2
# penalty in the objective, MSE over 8 columns, the single level 0.9
BIG_HEADS = ("q1_y1_pinball_nc0p1_m0", "q8_y1_pinball_nc2p2_m2", "q8_y8_pinball_nc2p2_m6", "q8_y8_mse_null_nc0p1_m1")
assert set(BIG_HEADS) <= {h["name"] for h in ec.HEADS}


def test_targets_are_distinct_and_planted_rows_dominate():
    """The targets are a distinct function of the row (a target paired with a neighbour's prediction, or with a far
    row's, is off by O(1) on average), and every planted row alone carries at least
    PLANTED_SHARE times the bound of every slot it feeds -- at every batch size, for the heads whose slots it feeds
    least (BIG_HEADS) from 65 536 rows on."""
    for B in ec.BATCH_SIZES:
        for head in ec.HEADS:
            if B > 1023 and head["name"] not in BIG_HEADS:
                continue
            rows, yp, y = _case(B, head)
            y0 = rows["y"][:, 0].astype(np.float64)
            if B > 1 and head is ec.HEADS[0]:          # (float32 values collide by chance among 10^6 rows: distinct up to that)
                assert len(np.unique(y0)) >= 0.99 * B
                for shift in (1, 7, B // 2):
                    assert np.abs(y0 - np.roll(y0, shift)).mean() >= 0.5, (B, shift)
            share = ec.planted_shares(yp, y, head, rows["planted"])
            assert share >= ec.PLANTED_SHARE, (B, head["name"], share)
            for b in rows["ties"]:
                assert np.any(y[b] == yp[b])


@pytest.mark.parametrize("B", ec.BATCH_SIZES)
def test_emulation_stays_inside_the_bound(B):
    """(a) every slot, every head; ROWS and BATCHES exact, the unused slots untouched."""
    worst = 0.0
    for head in ec.HEADS:
        rows, yp, y = _case(B, head)
        w = 1.0 / (B * head["Q"])
        failures, ratio = _judge(emulate(yp, y, head, w), yp, y, head, w)
        assert not failures, (B, head["name"], failures, ratio)
        worst = max(worst, ratio)
    print(f"B={B}: worst emulated error {worst:.3f} of the bound over {len(ec.HEADS)} heads")
    assert worst < 1.0


def test_accumulator_contract_in_the_emulation():
    """sentinels + two calls: the comparator accepts the sums and flags a touched unused slot, a NaN that the reference
    does not have, and a missing one."""
    head = ec.HEADS[6]
    start = np.array([3.25 + s for s in range(ec.EVAL_SLOTS)])
    got, add, bound = start.copy(), np.zeros(ec.EVAL_SLOTS), np.zeros(ec.EVAL_SLOTS)
    for B in (257, 1023):
        rows, yp, y = _case(B, head)
        got = emulate(yp, y, head, 0.37, start=got)
        a, _, b = ec.reference(yp, y, head, 0.37)
        add, bound = add + a, bound + b
    assert ec.compare_accumulator(got, start, add, bound, head["Q"])[0] == []
    bad = got.copy()
    bad[ec.EVAL_CHECK + head["Q"]] = np.nextafter(bad[ec.EVAL_CHECK + head["Q"]], 100.0)
    assert ec.compare_accumulator(bad, start, add, bound, head["Q"])[0] == [f"unused{ec.EVAL_CHECK + head['Q']}"]
    bad = got.copy()
    bad[ec.EVAL_SAE] = np.nan
    assert ec.compare_accumulator(bad, start, add, bound, head["Q"])[0] == ["sae"]
    nan_add = add.copy()
    nan_add[ec.EVAL_SAE] = np.nan
    assert ec.compare_accumulator(got, start, nan_add, bound, head["Q"])[0] == ["sae"]
    bad = got.copy()
    bad[ec.EVAL_ROWS] += 1
    assert ec.compare_accumulator(bad, start, add, bound, head["Q"])[0] == ["rows"]


# ------------------------------------------------------------------------------------------------ (b) the mutants
def _used(head):
    return {"objective", "sse", "sae"} | {f"check{q}" for q in range(head["Q"])}


@pytest.mark.parametrize("B", ec.BATCH_SIZES)
def test_mutant_drop_last_row(B):
    for head in (ec.HEADS[1], ec.HEADS[9], ec.HEADS[17]):
        rows, yp, y = _case(B, head)
        w = 1.0 / (B * head["Q"])
        failures, _ = _judge(emulate(yp, y, head, w, rows=B - 1), yp, y, head, w)
        assert set(failures) == _used(head) | {"rows"}, (B, head["name"], failures)


@pytest.mark.parametrize("B", [257, 65537, 262145])
def test_mutants_in_the_binned_order(B):
    """The window route: the metrics pass reads the rows in the binned order, and make_rows(binned=True) plants the rows
    that order puts at the loop edges -- so the mutants that lose a row there are caught on that route too."""
    head = ec.HEADS[13]
    rows = ec.make_rows(B, head["Q"], head["y_cols"], 5 + B % 1000, "permutation", binned=True)
    idx = rows["idx"]
    order = ec.binned_order(rows["coords"][idx], B)
    assert sorted(np.flatnonzero(np.isin(order, rows["planted"])).tolist()) == ec.planted_positions(B)
    assert ec.cell_grid(B) == {257: 32, 65537: 256, 262145: 256}[B] and not np.array_equal(order, np.arange(B))
    assert [ec.cell_grid(b) for b in (1, 64, 65, 256, 257, 65536, 65537, 1048576)] == [8, 8, 16, 16, 32, 256, 256, 256]
    rs = np.random.RandomState(B % 9973)
    yp = (0.7 * rs.standard_normal((B, head["Q"]))).astype(F32)
    y = rows["y"][idx]
    w = 1.0 / (B * head["Q"])
    assert _judge(emulate(yp[order], y[order], head, w), yp, y, head, w)[0] == []
    mutants = [dict(rows=B - 1)]
    if ec.rows_per_thread(B) > 1:
        mutants.append(dict(max_trips=1))
    if ec.partials_blocks(B) > ec.EVAL_T:
        mutants.append(dict(max_partials=ec.EVAL_T))
    for kw in mutants:
        failures, _ = _judge(emulate(yp[order], y[order], head, w, **kw), yp, y, head, w)
        assert _used(head) <= set(failures), (B, kw, failures)


@pytest.mark.parametrize("B", [b for b in ec.BATCH_SIZES if ec.rows_per_thread(b) > 1])
def test_mutant_drop_second_trip(B):
    for head in (ec.HEADS[0], ec.HEADS[7], ec.HEADS[13]):
        rows, yp, y = _case(B, head)
        w = 1.0 / (B * head["Q"])
        failures, _ = _judge(emulate(yp, y, head, w, max_trips=1), yp, y, head, w)
        assert set(failures) == _used(head), (B, head["name"], failures)


@pytest.mark.parametrize("B", [b for b in ec.BATCH_SIZES if ec.partials_blocks(b) > ec.EVAL_T])
def test_mutant_first_256_partials_only(B):
    for head in (ec.HEADS[1], ec.HEADS[8], ec.HEADS[18]):
        rows, yp, y = _case(B, head)
        w = 1.0 / (B * head["Q"])
        failures, _ = _judge(emulate(yp, y, head, w, max_partials=ec.EVAL_T), yp, y, head, w)
        assert set(failures) == _used(head), (B, head["name"], failures)


@pytest.mark.parametrize("B", [b for b in ec.BATCH_SIZES if b > 1])
def test_mutant_targets_in_sorted_order(B):
    """the predictions in the caller's order against the targets in the order a sort by coordinate leaves them"""
    for head in (ec.HEADS[3], ec.HEADS[6], ec.HEADS[12]):
        rows, yp, y = _case(B, head, kind="arange" if B > 1023 else "permutation")
        order = np.argsort(rows["coords"][rows["idx"], 0], kind="stable")
        assert not np.array_equal(order, np.arange(B))
        w = 1.0 / (B * head["Q"])
        failures, _ = _judge(emulate(yp, y[order], head, w), yp, y, head, w)
        assert set(failures) == _used(head), (B, head["name"], failures)


@pytest.mark.parametrize("B", [1, 257, 65537, 1048576])
def test_mutant_median_column_whatever_metric_col_says(B):
    heads = [h for h in ec.HEADS if h["metric_col"] != h["Q"] // 2]
    assert {h["Q"] for h in heads} == {2, 5, 8}
    for head in heads if B <= 65537 else heads[::4]:
        rows, yp, y = _case(B, head)
        w = 1.0 / (B * head["Q"])
        failures, _ = _judge(emulate(yp, y, head, w, metric_col=head["Q"] // 2), yp, y, head, w)
        assert set(failures) == {"sse", "sae"}, (B, head["name"], failures)


@pytest.mark.parametrize("B", [1, 257, 65537, 1048576])
def test_mutant_batch_weight_on_sse(B):
    for head in (ec.HEADS[0], ec.HEADS[10], ec.HEADS[15]):
        rows, yp, y = _case(B, head)
        for w in (1.0 / (B * head["Q"]), 0.999, 1.001):
            if w == 1.0:
                continue
            failures, _ = _judge(emulate(yp, y, head, w, weight_sse=True), yp, y, head, w)
            assert failures == ["sse"], (B, head["name"], w, failures)


@pytest.mark.parametrize("B", [1, 257, 65537])
def test_mutant_check_slot_at_index_q(B):
    for head in (h for h in ec.HEADS if h["Q"] < ec.MAX_Q):
        rows, yp, y = _case(B, head)
        w = 1.0 / (B * head["Q"])
        start = np.array([3.25 + s for s in range(ec.EVAL_SLOTS)])
        failures, _ = _judge(emulate(yp, y, head, w, start=start, stray_check=True), yp, y, head, w, start)
        assert failures == [f"unused{ec.EVAL_CHECK + head['Q']}"], (B, head["name"], failures)
        assert _judge(emulate(yp, y, head, w, start=start), yp, y, head, w, start)[0] == []
