"""The CPU side of the generated-dropout tests (tests/golden/dropout_cases.py), before any kernel is compared:
  * the replica of the mask contract (oracle/dropout.py): its vectorised and its scalar implementation agree, both
    reproduce stored known answers, and the masks have the statistics the contract implies;
  * the oracles carry masks: numpy and torch float64 agree with them, all-ones masks and p = 0 change nothing;
  * the comparison the GPU tests use (dropout_cases.compare) passes a float32 run with the right masks and FAILS
    each of the errors the GPU tests exist to catch;
  * the float64 references keep clear of the ReLU kinks (a condition on the input seeds, not on the kernels).
"""
import os

import numpy as np
import pytest

from golden import cases
from golden import dropout_cases as DC
from golden import shape_cases as SC
from oracle import dropout as drp
from oracle import stdadk_oracle as orc
from oracle import torch_f64

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _params64(cfg):
    return {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()}


# ------------------------------------------------------------------ the replica against itself
def test_thresholds_and_step_seed():
    for p, thr in DC.THRESHOLDS.items():
        assert drp.threshold(p) == thr
    assert drp.threshold(0.0) == 0 and drp.threshold(1.0) == 65536
    assert drp.step_seed(5, 0) == 5 and drp.step_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert drp.step_seed(2 ** 62 - 1, 3) == (2 ** 62 - 1 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64 < 2 ** 64
    assert drp.step_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C14


def test_vectorised_replica_equals_scalar_replica():
    """A few thousand (seed, step, layer, row, col): rows past 2^16 and 2^31, columns past 256, steps >= 1."""
    rs = np.random.RandomState(77)
    n = 0
    for seed in DC.SEEDS + (0, 2 ** 64 - 1):
        for step, layer in [(0, 0), (1, 0), (2, 7), (1000, 3)]:
            rows = np.concatenate([[0, 1, 299, 65535, 65536, 16320, 2 ** 31 - 1, 2 ** 31, 2 ** 33 + 7],
                                   rs.randint(0, 2 ** 20, 6)]).astype(np.int64)
            h = 330
            hv, bits = drp.hash_bits(seed, step, layer, rows, h)
            masks = {p: drp.keep_mask(seed, step, layer, rows, h, p) for p in DC.THRESHOLDS}
            for i in rs.randint(0, len(rows), 12):
                for c in np.concatenate([[0, 63, 64, 127, 128, 256, 319, 329], rs.randint(0, h, 4)]):
                    hs = drp.hash_scalar(seed, step, layer, rows[i], c)
                    assert int(hv[i, c]) == hs, (seed, step, layer, rows[i], c)
                    assert int(bits[i, c]) == ((hs >> 16) if c & 64 else (hs & 0xFFFF))
                    for p, mk in masks.items():
                        assert bool(mk[i, c]) == drp.keep_scalar(seed, step, layer, rows[i], c, p)
                    n += 1
    assert n >= 2000
    # the pair trick: columns c and c + 64 of a 128-column block read ONE hash, no other two columns do
    hv, _ = drp.hash_bits(5, 0, 0, np.arange(4), 384)
    for c in range(384):
        same = [d for d in range(384) if d != c and np.array_equal(hv[:, c], hv[:, d])]
        assert same == [c ^ 64], (c, same)


def test_known_answers():
    g = np.load(os.path.join(GOLD, "dropout_known_answers.npz"))
    assert len(g["seed"]) >= 20
    for seed, step, layer, row, col, p, hv, keep in zip(*(g[k] for k in ("seed", "step", "layer", "row", "col", "p",
                                                                         "hash", "keep"))):
        args = (int(seed), int(step), int(layer), int(row), int(col))
        assert drp.hash_scalar(*args) == int(hv), args
        assert drp.keep_scalar(*args, float(p)) == bool(keep), args
        vec_h, _ = drp.hash_bits(args[0], args[1], args[2], np.array([args[3]], np.int64), args[4] + 1)
        assert int(vec_h[0, args[4]]) == int(hv), args
        assert bool(drp.keep_mask(args[0], args[1], args[2], np.array([args[3]], np.int64), args[4] + 1, float(p))[0, -1]) \
            == bool(keep), args
    assert g["keep"].any() and not g["keep"].all()


def test_window_rows_is_the_inverse_of_the_stable_sort():
    coords = cases.make_inputs(DC.config(DC.ENTRIES[2]))[1]
    perm = drp.window_order(coords, 32)
    pos = drp.window_rows(coords, 32)
    keys = orc.cell_keys(coords, 32)
    assert np.array_equal(np.sort(perm), np.arange(len(coords))) and np.array_equal(perm[pos], np.arange(len(coords)))
    assert np.all(np.diff(keys[perm]) >= 0) and not np.array_equal(pos, np.arange(len(coords)))
    same = np.diff(keys[perm]) == 0
    assert same.any() and np.all(np.diff(perm)[same] > 0)         # ascending caller index inside a cell
    assert np.array_equal(DC.row_keys(coords, False), np.arange(len(coords)))
    assert np.array_equal(DC.row_keys(coords, True), drp.window_rows(coords, 32))      # pick_cell_grid(300) == 32


# ------------------------------------------------------------------ statistics of the contract
def _corr_z(a, b, q):
    """z-score of the sample correlation of two Bernoulli(q) arrays under independence."""
    a, b = a.ravel().astype(np.float64), b.ravel().astype(np.float64)
    return abs(((a - q) * (b - q)).mean()) / (q * (1 - q)) * np.sqrt(a.size)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_mask_statistics(p):
    """With q = 1 - threshold / 65536 and independent uniform 16-bit fields: keep rate overall, per column and per row,
    and no correlation between the two halves of a hash, adjacent rows, layers or steps.  Bounds in standard
    deviations, derived (5 overall and per correlation, 6 for the maxima over 256 columns / 4 096 rows of 27 masks)."""
    B, h = 4096, 256
    q = 1.0 - drp.threshold(p) / 65536.0
    sd = np.sqrt(q * (1 - q))
    rows = np.arange(B)
    worst = dict(overall=0.0, col=0.0, row=0.0, pair=0.0, rows=0.0, layers=0.0, steps=0.0)
    total, count = 0.0, 0
    for seed in DC.SEEDS:
        mk = {(st, l): drp.keep_mask(seed, st, l, rows, h, p) for st in range(3) for l in range(3)}
        for m in mk.values():
            total += m.sum()
            count += m.size
            worst["col"] = max(worst["col"], np.abs(m.mean(0) - q).max() / (sd / np.sqrt(B)))
            worst["row"] = max(worst["row"], np.abs(m.mean(1) - q).max() / (sd / np.sqrt(h)))
            lo = m.reshape(B, h // 128, 2, 64)
            worst["pair"] = max(worst["pair"], _corr_z(lo[:, :, 0], lo[:, :, 1], q))
            worst["rows"] = max(worst["rows"], _corr_z(m[:-1], m[1:], q))
        for st in range(3):
            for a, b in ((0, 1), (0, 2), (1, 2)):
                worst["layers"] = max(worst["layers"], _corr_z(mk[(st, a)], mk[(st, b)], q))
                worst["steps"] = max(worst["steps"], _corr_z(mk[(a, st)], mk[(b, st)], q))
    worst["overall"] = abs(total / count - q) / (sd / np.sqrt(count))
    print(f"p {p}: q {q:.6f}, z-scores {', '.join(f'{k} {v:.2f}' for k, v in worst.items())}")
    assert worst["overall"] <= 5
    assert worst["col"] <= 6 and worst["row"] <= 6
    for k in ("pair", "rows", "layers", "steps"):
        assert worst[k] <= 5, k


def test_threshold_one_drops_only_zero_fields():
    _, bits = drp.hash_bits(5, 0, 0, np.arange(4096), 256)
    m = drp.keep_mask(5, 0, 0, np.arange(4096), 256, 1e-5)
    assert np.array_equal(~m, bits == 0) and 1 <= (~m).sum() <= 60          # 16 expected of 2^20


# ------------------------------------------------------------------ the oracles with masks
def _rel(a, b):
    return float(DC.rel_l2(a, b))


@pytest.mark.parametrize("e", [DC.ENTRIES[2], DC.ENTRIES[3], DC.ENTRIES[6]], ids=DC.entry_id)
def test_float64_oracles_agree_with_masks(e):
    """numpy and chunked torch float64 with the same masks, as test_torch_f64_oracle.py (chunks cut the masks); a wide
    kink band so that the single-row re-evaluations run with their row of the masks."""
    cfg = DC.config(e)
    inp = SC.make_inputs(cfg)
    params = _params64(cfg)
    mk = DC.masks(cfg, DC.entry_seed(e), 1, DC.row_keys(inp[1], e[0] in DC.WINDOW_CASES))
    tol = 1e-3
    yo, lo, go, ao = orc.train_step_grads(*inp, params, cfg, kink_tol=tol, drop_masks=mk, drop_p=cfg["dropout"])
    yt, lt, gt, at = torch_f64.train_step_grads(*inp, params, cfg, device="cpu", chunk=128, kink_tol=tol,
                                                drop_masks=mk, drop_p=cfg["dropout"])
    assert _rel(yt, yo) <= 1e-12 and abs(lt - lo) <= 1e-12 * lo
    for k in go:
        assert _rel(gt[k], go[k]) <= 1e-12, (k, _rel(gt[k], go[k]))
    assert len(ao) > 0 and [u for u, _ in at] == sorted(u for u, _ in ao)
    do = dict(ao)
    dropped = 0
    for u, d in at:
        li, r, c = u
        norm = sum(float(np.abs(v).sum()) for v in do[u].values())
        dropped += not mk[li][r, c]
        assert (norm == 0.0) == (not mk[li][r, c]), u             # a dropped unit's ReLU side changes nothing
        for k in d:
            assert np.linalg.norm(d[k] - do[u][k]) <= 1e-10 * max(np.linalg.norm(do[u][k]), 1e-300), (u, k)
    assert dropped > 0 or len(at) < 20                             # (about one in ten is dropped)
    # and the masks matter: the unmasked oracle is somewhere else
    y0 = orc.train_step_grads(*inp, params, cfg)[0]
    assert _rel(y0, yo) > 1e-2


@pytest.mark.parametrize("e", [DC.ENTRIES[1], DC.ENTRIES[2]], ids=DC.entry_id)
def test_all_ones_masks_and_zero_p_are_the_plain_oracle(e):
    cfg = DC.config(e)
    inp = SC.make_inputs(cfg)
    params = _params64(cfg)
    ones = [np.ones((cfg["B"], h), bool) for h in cfg["hidden_dims"]]
    some = DC.masks(cfg, 5, 0, np.arange(cfg["B"]))
    plain = orc.train_step_grads(*inp, params, cfg, kink_tol=1e-3)
    tplain = torch_f64.train_step_grads(*inp, params, cfg, chunk=128, kink_tol=1e-3)
    for fn, ref, kw in ((orc.train_step_grads, plain, {}), (torch_f64.train_step_grads, tplain, dict(chunk=128))):
        for mk, p in ((some, 0.0), (None, 0.3)):
            y, l, g, a = fn(*inp, params, cfg, kink_tol=1e-3, drop_masks=mk, drop_p=p, **kw)
            assert np.array_equal(y, ref[0]) and l == ref[1]
            for k in g:
                assert np.array_equal(g[k], ref[2][k]), k
            assert [u for u, _ in a] == [u for u, _ in ref[3]]
            for (_, d0), (_, d1) in zip(a, ref[3]):
                for k in d0:
                    assert np.array_equal(d0[k], d1[k]), k
    # all-ones masks at p > 0: exactly the plain network scaled by 1 / (1 - p) per layer -- p = 0.5 scales by 2, a
    # power of two, so every float64 product is exact; undone by halving each hidden layer's outgoing weights
    half = dict(params)
    layers, _, keys = orc.split_params(params, len(cfg["hidden_dims"]), cfg["layernorm"])
    lin = [k for k in sorted(keys) if params[f"mlp.{k}.weight"].ndim == 2][1:]
    for k in lin:
        half[f"mlp.{k}.weight"] = params[f"mlp.{k}.weight"] * 0.5
    y1 = orc.model_forward(*inp[:3], half, cfg, drop_masks=ones, drop_p=0.5)[0]
    assert np.array_equal(y1, plain[0])


# ------------------------------------------------------------------ teeth of the comparison
TEETH = DC.ENTRIES[2]          # w_k80_k176_noln, 300 rows, p = 0.1: three layers on the window path


def _f32_run(cfg, inp, fwd, bwd=None, scale_one=False):
    """A float32 numpy forward + backward with keep-masks `fwd` in the forward and `bwd` (default: the same) in the
    backward; `scale_one`: kept values are not scaled."""
    X, coords, t, y = inp
    p = cfg["dropout"]
    st = cases.make_state(cfg)
    nh, ln = len(cfg["hidden_dims"]), cfg["layernorm"]
    f = (lambda m: np.asarray(m, np.float32) * np.float32(1.0 - p)) if scale_one else (lambda m: m)
    yp, cache, *_ = orc.model_forward(X, coords, t, st, cfg, dtype=np.float32, drop_masks=[f(m) for m in fwd], drop_p=p)
    if bwd is not None:
        sc = np.float32(1.0) if scale_one else np.float32(1.0 / (1.0 - p))
        cache = [c[:4] + (np.asarray(m, np.float32) * sc,) for c, m in zip(cache[:-1], bwd)] + [cache[-1]]
    grads = orc.mlp_mse_backward(yp, y, cache, st, nh, ln, dtype=np.float32)
    d = yp.astype(np.float64) - y
    return yp, float((d * d).mean()), grads


def test_comparison_has_teeth():
    e = TEETH
    assert e[0] == "w_k80_k176_noln" and e[1] == 300 and e[2] == 0.1
    cfg = DC.config(e)
    inp = SC.make_inputs(cfg)
    seed, step = DC.entry_seed(e), 1
    hd = cfg["hidden_dims"]
    rows = DC.row_keys(inp[1], True)
    ref = DC.reference(cfg, inp, _params64(cfg), seed, step, True)
    good = DC.masks(cfg, seed, step, rows)
    print("float32 run with the contract's masks:")
    DC.compare(*_f32_run(cfg, inp, good), ref)

    next_layer = [m.copy() for m in good]
    next_layer[1] = drp.keep_mask(seed, step, 2, rows, hd[1], e[2])
    swapped = [m.copy() for m in good]
    swapped[0][:, [5, 69]] = swapped[0][:, [69, 5]]
    variants = {
        "backward mask of layer 1 keyed with layer_id + 1": dict(fwd=good, bwd=next_layer),
        "rows shifted by one": dict(fwd=DC.masks(cfg, seed, step, rows + 1)),
        "low and high half swapped for one pair": dict(fwd=swapped),
        "masks of step s at step s + 1": dict(fwd=DC.masks(cfg, seed, step - 1, rows)),
        "scale 1 instead of 1 / (1 - p)": dict(fwd=good, bwd=good, scale_one=True),
        "caller order where sorted order is meant": dict(fwd=DC.masks(cfg, seed, step, DC.row_keys(inp[1], False))),
    }
    for name, kw in variants.items():
        print(name + ":")
        with pytest.raises(AssertionError):
            DC.compare(*_f32_run(cfg, inp, **kw), ref)
    # the backward-only error leaves y and the loss alone: only the gradients can show it
    yb, lb, _ = _f32_run(cfg, inp, good, next_layer)
    yg, lg, _ = _f32_run(cfg, inp, good)
    assert np.array_equal(yb, yg) and lb == lg


# ------------------------------------------------------------------ near-kink cap
def _small(entries):
    return [e for e in entries if e[1] == DC.SMALL_B]


def _kink_counts(e):
    """Units within KINK_TOL of a ReLU kink in every 300-row float64 reference test_gpu_dropout.py builds for an entry:
    the module runs (step 0, sorted and caller rows, the seed torch draws after manual_seed(entry index)) and
    STEPS one-call steps along the float64 trajectory of clip + AdamW + EMA."""
    import torch
    cfg = DC.config(e)
    inp = SC.make_inputs(cfg)
    window = e[0] in DC.WINDOW_CASES
    torch.manual_seed(DC.ENTRIES.index(e))
    mseed = int(torch.randint(0, 2 ** 62, (1,)).item())
    counts = {}
    for label, w in (("module", window), ("module dense", False)):
        counts[label] = len(DC.reference(cfg, inp, _params64(cfg), mseed, 0, w)[3])
    seed = DC.entry_seed(e)
    params = _params64(cfg)
    o = cases.OPT
    mm = {k: np.zeros_like(v) for k, v in params.items()}
    vv = {k: np.zeros_like(v) for k, v in params.items()}
    sh = {k: v.copy() for k, v in params.items()}
    clip = None
    for s in range(DC.STEPS):
        yo, lo, go, alts = DC.reference(cfg, inp, params, seed, s, window)
        counts[f"step {s}"] = len(alts)
        if clip is None:
            clip = DC.CLIP_OF_NORM * float(np.sqrt(sum(float((g * g).sum()) for g in go.values())))
        orc.adamw_ema_step(params, go, mm, vv, sh, s + 1, o["lr"], o["weight_decay"], o["betas"], DC.ADAM_EPS, clip,
                           o["ema_decay"])
    if e == TEETH:
        counts["teeth"] = len(DC.reference(cfg, inp, _params64(cfg), seed, 1, window)[3])
    return counts


@pytest.mark.parametrize("e", _small(DC.ENTRIES), ids=DC.entry_id)
def test_float64_references_avoid_kinks(e):
    """At most MAX_NEAR_KINK such units in every 300-row reference; an entry that exceeds it gets another input seed
    (dropout_cases.INPUT_SEED), never a wider cap."""
    counts = _kink_counts(e)
    print(f"{DC.entry_id(e)}: units within {DC.KINK_TOL} of a kink: {counts}")
    assert max(counts.values()) <= DC.MAX_NEAR_KINK, counts


def test_rank_references_avoid_kinks():
    e = DC.ENTRIES[DC.RANK_ENTRY]
    cfg = DC.config(e)
    inp = SC.make_inputs(cfg)
    for rank in (0, 1):
        seed = (DC.RANK_BASE_SEED + 0xD1B54A32D192ED03 * rank) % 2 ** 64
        alts = DC.reference(cfg, inp, _params64(cfg), seed, 0, e[0] in DC.WINDOW_CASES)[3]
        assert len(alts) <= DC.MAX_NEAR_KINK, (rank, len(alts))
