"""Cases, inputs, the float64 reference and the error bound of the per-batch validation tests
(tests/test_gpu_eval_batches.py; the CPU half with the float32 emulation and the mutants: tests/test_eval_cases_cpu.py).

Numpy only and deterministic, like cases.py: the GPU box rebuilds every input.

What is pinned is stdadk_eval_indexed_f32's metrics pass (csrc/eval.hip): eval_partials_kernel -- one thread per row,
grid-stride over at most EVAL_MAX_WG workgroups of EVAL_T threads, float sums per thread, a 64-lane wave sum, the four
wave sums of a workgroup added in double -- and eval_finish_kernel, one workgroup whose thread i adds the partials
i, i + 256, ... in double.

The reduction bound (first order in u = 2^-24, derived from that order of operations, not measured):

    |got - ref| <= (a + 6 + c) u sum|term|

  a   additions into one thread's float accumulator: rows_per_thread(B) for SSE, SAE and each CHECK slot,
      rows_per_thread(B) * Q for the objective (Q element terms per row);
  6   the levels of the 64-lane wave sum;
  c   roundings that form one element term from exact float32 inputs (ROUNDINGS below, counted from csrc/loss.h and
      the kernel's row body):
        SSE        d = p - y (1), d * d: the error of d twice plus the product's own rounding where the compiler does not
                   contract it into the accumulator's fma                                                   -> 3
        SAE        d = p - y                                                                                 -> 1
        CHECK      e = y - p (1), tau - 1 (1), the product with e (1); max() selects, it does not round     -> 3
        OBJECTIVE  MSE: as SSE -> 3.  Pinball: the check term (3) next to w f with w = nc_w * Q (1), f = d or d * d
                   (1 or 3), both terms non-negative, then the fma's rounding of their sum (1)              -> 5
  everything after the wave sum is double (2^-53) and contributes nothing at this scale.
`ref` and `sum|term|` are float64 sums over the float32 predictions the call RETURNED and the float32 targets at idx:
the forward's own error is not in this comparison (it has its own bound, 1e-5 of max(1, max|y|), per prediction).
"""
import math

import numpy as np

from golden import cases

EVAL_T = 256                 # csrc/eval.hip
EVAL_MAX_WG = 1024           # csrc/loss.h
WAVE = 64
MAX_Q = 8                    # STDADK_MAX_Q
# include/stdadk.h
EVAL_OBJECTIVE, EVAL_SSE, EVAL_SAE, EVAL_ROWS, EVAL_BATCHES, EVAL_CHECK, EVAL_SLOTS = 0, 1, 2, 3, 4, 5, 16
ULP = 2.0 ** -24
TREE_LEVELS = 6
ROUNDINGS = {"sse": 3, "sae": 1, "check": 3, "objective": 5}
assert max(ROUNDINGS.values()) <= 8 and 2 ** TREE_LEVELS == WAVE and EVAL_T == 4 * WAVE
PLANTED_SHARE = 100.0        # a planted row alone carries at least this multiple of the bound of every slot it feeds


def partials_blocks(B):
    """eval_partials_blocks: workgroups (= partials per value) of a batch of B rows."""
    return min(-(-max(int(B), 1) // EVAL_T), EVAL_MAX_WG)


def stride(B):
    """Rows between two trips of one thread through eval_partials_kernel's row loop."""
    return partials_blocks(B) * EVAL_T


def rows_per_thread(B):
    """Trips of thread 0 of workgroup 0 (the most any thread makes) through the row loop."""
    return max(1, -(-int(B) // stride(B)))


# The smallest sizes that reach every branch of the two kernels (the property each one has is asserted below, so a
# change of EVAL_T / EVAL_MAX_WG fails here on the CPU instead of silently un-testing an edge).
BATCH_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 65536, 65537, 262144, 262145, 1048576)
BIG = 65536                  # from here on the float64 forward is checked on a sample of the rows
FORWARD_SAMPLE = 4096


def check_table():
    """The edges BATCH_SIZES claims, restated from the constants."""
    T, W, M = EVAL_T, WAVE, EVAL_MAX_WG
    assert BATCH_SIZES[0] == 1 and partials_blocks(1) == 1 and partials_blocks(0) == 1
    assert {W - 1, W, W + 1} <= set(BATCH_SIZES)                       # wave edge
    assert {T - 1, T, T + 1} <= set(BATCH_SIZES)                       # workgroup edge
    assert partials_blocks(T) == 1 and partials_blocks(T + 1) == 2
    assert 1023 in BATCH_SIZES and 1023 % W and 1023 % T and partials_blocks(1023) == 4
    assert partials_blocks(65536) == T                                 # one partial per finishing thread
    assert partials_blocks(65537) == T + 1                             # the finishing loop strides
    assert partials_blocks(262144) == M and rows_per_thread(262144) == 1 and 262144 == M * T
    assert partials_blocks(262145) == M and rows_per_thread(262145) == 2
    assert 262145 - stride(262145) == 1                                # exactly one thread makes the second trip
    assert 1048576 == 4 * M * T and rows_per_thread(1048576) == 4     # val_batch_size(65536, n): 16 * 65536 rows
    assert all(rows_per_thread(b) == 1 for b in BATCH_SIZES if b <= M * T)
    assert all(b < 2 ** 31 for b in BATCH_SIZES)
    for B in BATCH_SIZES:
        assert all(0 <= r < B for r in planted_positions(B))
        assert not set(planted_positions(B)) & set(tie_positions(B))
    qs = {h["Q"] for h in HEADS}
    assert qs == {1, 2, 5, 8} and max(qs) == MAX_Q
    assert {(h["Q"], h["y_cols"]) for h in HEADS} >= {(q, c) for q in qs for c in (1, q)}
    kinds = {(h["kind"], h["y_cols"] == h["Q"]) for h in HEADS if h["Q"] > 1}
    assert ("mse_null", True) in kinds and ("mse", False) in kinds
    assert {(h["nc_power"]) for h in HEADS if h["kind"] == "pinball" and h["nc_weight"] > 0 and h["Q"] > 1} == {1, 2}
    for q in (5, 8):
        assert {h["metric_col"] for h in HEADS if h["Q"] == q} == set(range(q))
    for h in HEADS:
        assert 0 <= h["metric_col"] < h["Q"] and h["y_cols"] in (1, h["Q"])
        assert h["kind"] != "mse_null" or h["y_cols"] == h["Q"]       # a NULL descriptor means targets [B, Q]
    assert len({h["name"] for h in HEADS}) == len(HEADS)
    assert set(INDEX_KINDS) == {"arange", "reversed", "permutation", "subset", "all_same", "few_repeated"}


def _head(Q, y_cols, kind, nc_weight, nc_power, metric_col):
    return dict(name=f"q{Q}_y{y_cols}_{kind}_nc{nc_weight:g}p{nc_power}_m{metric_col}", Q=Q, y_cols=y_cols, kind=kind,
                nc_weight=nc_weight, nc_power=nc_power, metric_col=metric_col)


# (Q, y_cols, loss kind, nc_weight, nc_power, metric_col).  Kinds: "mse_null" = MSE through a NULL descriptor (targets
# [B, Q]), "mse" = the MSE descriptor (y_cols == 1: one target broadcast over the Q outputs), "pinball".
HEADS = [_head(*h) for h in (
    (1, 1, "mse_null", 0.0, 1, 0), (1, 1, "pinball", 0.0, 1, 0),
    (2, 2, "mse_null", 0.0, 1, 1), (2, 1, "mse", 0.0, 1, 0), (2, 1, "pinball", 0.5, 1, 1), (2, 2, "pinball", 2.0, 2, 0),
    (5, 1, "pinball", 0.5, 1, 0), (5, 5, "pinball", 2.0, 2, 1), (5, 1, "mse", 0.0, 1, 2), (5, 5, "mse_null", 0.0, 1, 3),
    (5, 1, "pinball", 2.0, 2, 4),
    (8, 1, "pinball", 0.5, 1, 0), (8, 8, "mse_null", 0.0, 1, 1), (8, 1, "pinball", 2.0, 2, 2), (8, 1, "mse", 0.0, 1, 3),
    (8, 8, "pinball", 0.5, 1, 4), (8, 1, "pinball", 0.0, 1, 5), (8, 8, "pinball", 2.0, 2, 6), (8, 1, "pinball", 0.5, 1, 7),
)]


def head_taus(head):
    """Quantile levels of a head as float32 (what the descriptor holds); 0.5 throughout without a pinball descriptor."""
    Q = head["Q"]
    if head["kind"] != "pinball":
        return np.full(Q, 0.5, np.float32)
    return np.array([0.9], np.float32) if Q == 1 else np.linspace(0.05, 0.95, Q).astype(np.float32)


INDEX_KINDS = ("arange", "reversed", "permutation", "subset", "all_same", "few_repeated")


def resident_rows(kind, B):
    """Rows of the resident arrays a batch of B rows of this kind indexes into."""
    return B + B // 2 + 3 if kind == "subset" else B


def make_index(kind, B, seed):
    """idx (B,) int64 into resident_rows(kind, B) rows."""
    if kind == "arange":
        return np.arange(B, dtype=np.int64)
    if kind == "reversed":
        return np.arange(B, dtype=np.int64)[::-1].copy()
    if kind == "permutation":
        return np.random.RandomState(seed + 7).permutation(B).astype(np.int64)
    if kind == "subset":
        return np.random.RandomState(seed + 7).permutation(resident_rows(kind, B))[:B].astype(np.int64)
    if kind == "all_same":
        return np.full(B, B // 2, dtype=np.int64)
    if kind == "few_repeated":
        return np.arange(B, dtype=np.int64) % 7
    raise KeyError(kind)


def cell_grid(B):
    """pick_cell_grid (csrc/window.hip): cells per axis of the window path's binning of a batch of B rows."""
    G = 8
    while G < 256 and G * G < B:
        G <<= 1
    return G


def binned_order(coords, B):
    """The window path's row order (the order eval_partials_kernel reads predictions and targets in on that route):
    order[r] = batch position of sorted row r.  Cells ascending by cx * G + cy, cx = clamp(floor(fl32(x * G)), 0, G - 1),
    inside a cell by batch position (cell_order_kernel ranks by index) -- the integer contract
    test_gpu_parity.test_bin_obs_bit_exact pins.  `coords`: the (B, 2) float32 coordinates at idx."""
    G = cell_grid(B)
    c = np.asarray(coords, np.float32)
    assert c.shape == (B, 2)
    cell = []
    for a in (0, 1):
        f = np.floor((c[:, a] * np.float32(G)).astype(np.float32))
        cell.append(np.clip(np.where(np.isnan(f), 0.0, f), 0, G - 1).astype(np.int64))
    return np.argsort(cell[0] * G + cell[1], kind="stable")


def planted_positions(B):
    """Batch positions where a loop of the two kernels can lose a row: the first, both sides of the first workgroup
    edge, both sides of the grid-stride edge, the last."""
    s = stride(B)
    return sorted({r for r in (0, EVAL_T - 1, EVAL_T, s - 1, s, B - 1) if 0 <= r < B})


def tie_positions(B, planted=None):
    """A handful of batch positions whose targets the GPU test sets equal to the returned predictions."""
    planted = set(planted_positions(B) if planted is None else planted)
    return [r for r in (1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29) if r < B and r not in planted][:5]


def planted_offset(B):
    """Target offset of a planted row, a power of two.  The slot a planted row feeds least is a check-loss slot at
    tau = 0.05 (or 0.95 on the other side): 0.05 D against a bound of (a + 6 + 3) u sum|term| with sum|term| below
    B (|e| is O(1), tau <= 1).  D = 2^ceil(log2(4 PLANTED_SHARE (a + 9) u B / 0.05)), at least 64 (the 4: head room for
    the objective's non-crossing terms and for |e| above 1); the share is asserted from the terms themselves by
    planted_shares()."""
    need = 4.0 * PLANTED_SHARE * (rows_per_thread(B) + TREE_LEVELS + 3) * ULP * B / 0.05
    return float(2.0 ** max(6, math.ceil(math.log2(need))))


_INPUTS = {}


def _inputs(cfg):
    """cases.make_inputs, the last few results kept (the heads of one batch size share their rows)."""
    key = repr(sorted(cfg.items()))
    if key not in _INPUTS:
        while len(_INPUTS) >= 4:
            _INPUTS.pop(next(iter(_INPUTS)))
        _INPUTS[key] = cases.make_inputs(cfg)
    return _INPUTS[key]


def make_rows(B, Q, y_cols, seed, kind="arange", cfg=None, binned=False):
    """Resident arrays and the index of one case, built on cases.make_inputs (its edge coordinates first):
      X, coords, t   float32, resident_rows(kind, B) rows
      y              (rows, y_cols) float32: make_inputs' target plus a golden-ratio sequence of the row number (any two
                     rows differ at O(1) in expectation: a target paired with another row's prediction shows at O(1)
                     per row) plus 0.25 per column; the planted rows carry +-planted_offset(B), signs alternating
      idx            (B,) int64 of `kind`
      planted, ties  batch positions (planted: their resident rows idx[pos] carry the offset, once per distinct row;
                     ties: tie_positions(B), none for "all_same").  `binned`: the planted rows are the batch positions
                     that binned_order() puts AT planted_positions(B), for the route whose metrics pass walks the
                     binned order
    """
    cfg = dict(cfg if cfg is not None else cases.MODEL_CASES["tiny9"])
    R = resident_rows(kind, B)
    cfg.update(B=R, seed=seed)
    X, coords, t, y0 = _inputs(cfg)
    r = np.arange(R, dtype=np.float64)
    spread = 2.0 * ((r * 0.6180339887498949) % 1.0) - 1.0
    y = y0.astype(np.float64) + spread[:, None] + 0.25 * np.arange(y_cols, dtype=np.float64)[None, :]
    idx = make_index(kind, B, seed)
    planted, D = planted_positions(B), planted_offset(B)
    if binned:
        order = binned_order(coords[idx], B)
        planted = sorted(int(order[r]) for r in planted)
    seen = set()
    for k, pos in enumerate(planted):
        row = int(idx[pos])
        if row not in seen:
            y[row] += D if k % 2 == 0 else -D
            seen.add(row)
    ties = [] if kind == "all_same" else tie_positions(B, planted)  # (one row for all: a tie would zero every term)
    return dict(X=X, coords=coords, t=t, y=y.astype(np.float32), idx=idx, planted=planted, ties=ties, offset=D)


def set_ties(y, idx, yp, ties):
    """Exact ties at the kink of the check loss: the targets of the batch positions `ties` become the predictions
    the pass returned for them (column b % Q of row b under broadcast targets, the whole row under column targets).
    `y` (the resident targets) is changed in place."""
    Q = yp.shape[1]
    for b in ties:
        y[idx[b]] = yp[b] if y.shape[1] == Q and Q > 1 else yp[b, b % Q]


# ------------------------------------------------------------------------------------------------ float64 reference
def slot_terms(yp, y, head):
    """Per-row element terms of every value the pass sums, float64 from float32 predictions yp (B, Q) and the targets
    y (B, y_cols) of the SAME rows: {"sse": (B,), "sae": (B,), "objective": (B, Q), "check": (B, Q)}."""
    yp = np.asarray(yp, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    B, Q = yp.shape
    assert Q == head["Q"] and y.shape == (B, head["y_cols"])
    yt = np.broadcast_to(y, (B, Q)) if y.shape[1] == 1 else y
    mc = head["metric_col"]
    d = yp[:, mc] - yt[:, mc]
    tau = head_taus(head).astype(np.float64)[None, :]
    e = yt - yp
    check = np.maximum((tau - 1.0) * e, tau * e)
    if head["kind"] == "pinball":
        obj = check.copy()
        if head["nc_weight"] > 0 and Q > 1:
            gap = np.maximum(yp[:, :-1] - yp[:, 1:], 0.0)
            w = float(np.float32(head["nc_weight"])) * Q
            obj[:, :-1] += w * (gap if head["nc_power"] == 1 else gap * gap)
    else:
        obj = (yp - yt) ** 2
    return {"sse": d * d, "sae": np.abs(d), "objective": obj, "check": check}


def reference(yp, y, head, batch_weight):
    """(add, mag, bound): what one call adds to each of the EVAL_SLOTS accumulator slots in float64, the sum of the
    absolute terms behind each slot, and the reduction bound of each slot (0 for ROWS, BATCHES and the unused slots:
    exact)."""
    B, Q = np.asarray(yp).shape
    terms = slot_terms(yp, y, head)
    a = rows_per_thread(B)
    add, mag, bound = (np.zeros(EVAL_SLOTS) for _ in range(3))

    def put(slot, term, adds, c, w=1.0):
        add[slot] = w * term.sum()
        mag[slot] = abs(w) * np.abs(term).sum()
        bound[slot] = (adds + TREE_LEVELS + c) * ULP * mag[slot]

    put(EVAL_OBJECTIVE, terms["objective"], a * Q, ROUNDINGS["objective"], batch_weight)
    put(EVAL_SSE, terms["sse"], a, ROUNDINGS["sse"])
    put(EVAL_SAE, terms["sae"], a, ROUNDINGS["sae"])
    for q in range(Q):
        put(EVAL_CHECK + q, terms["check"][:, q], a, ROUNDINGS["check"])
    add[EVAL_ROWS], add[EVAL_BATCHES] = float(B), 1.0
    return add, mag, bound


def slot_names(Q):
    return {EVAL_OBJECTIVE: "objective", EVAL_SSE: "sse", EVAL_SAE: "sae", EVAL_ROWS: "rows", EVAL_BATCHES: "batches",
            **{EVAL_CHECK + q: f"check{q}" for q in range(Q)}}


def compare_accumulator(got, start, add, bound, Q):
    """The comparator of both halves.  `got`: the accumulator after the call(s); `start`: what it held before; `add`,
    `bound`: sums over the calls of reference()'s.  Returns (failures, worst): the names of the slots outside their
    bound -- a used slot off by more than its bound, or NaN where the reference is not (or the reverse); ROWS or
    BATCHES not the exact sum; an unused slot whose BITS differ from `start` -- and the largest error / bound over the
    used slots with a non-zero bound."""
    got, start = np.asarray(got, np.float64), np.asarray(start, np.float64)
    assert got.shape == start.shape == (EVAL_SLOTS,)
    names = slot_names(Q)
    failures, worst = [], 0.0
    for s in range(EVAL_SLOTS):
        if s in (EVAL_ROWS, EVAL_BATCHES):
            if got[s] != start[s] + add[s]:
                failures.append(names[s])
        elif s in names:
            want = start[s] + add[s]
            if np.isnan(want) or np.isnan(got[s]):
                if not (np.isnan(want) and np.isnan(got[s])):
                    failures.append(names[s])
                continue
            err = abs(got[s] - want)
            if not err <= bound[s]:
                failures.append(names[s])
            if bound[s] > 0:
                worst = max(worst, err / bound[s])
        elif got[s:s + 1].view(np.int64)[0] != start[s:s + 1].view(np.int64)[0]:
            failures.append(f"unused{s}")
    return failures, worst


def planted_shares(yp, y, head, planted):
    """Smallest (term of one planted row) / (reduction bound of the slot) over the planted rows and the slots they feed
    (batch_weight scales both alike and drops out)."""
    terms = slot_terms(yp, y, head)
    _, _, bound = reference(yp, y, head, 1.0)
    Q = head["Q"]
    worst = math.inf
    for r in planted:
        worst = min(worst, terms["objective"][r].sum() / bound[EVAL_OBJECTIVE], terms["sse"][r] / bound[EVAL_SSE],
                    terms["sae"][r] / bound[EVAL_SAE],
                    min(terms["check"][r, q] / bound[EVAL_CHECK + q] for q in range(Q)))
    return worst


check_table()
