"""Grid scores on the device: stdadk_grid_score_f32 alone against a numpy float64 restatement written here (every
element term formed in double from the float32 operands, as the kernel does), its accumulation across chunks and its
determinism; Predictor.score_grid against the scores of predict_grid's own output on the three layer-0 paths, chunked
and not; grid_scores against Evaluator; refused arguments."""
import numpy as np
import pytest
import torch

from golden import cases
import test_gpu_parity as T

pytestmark = pytest.mark.gpu
TAUS = [0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.95]


def sums64(y, z, code, mcol, taus, lo, hi):
    """(split (4,16), site (4,S,3), time (4,nT,3)) float64 from y (nT*S,Q), z (nT,S), code (nT,S); levels as float32."""
    nT, S = z.shape
    Q = y.shape[1]
    p = y.astype(np.float64).reshape(nT, S, Q)
    zd = z.astype(np.float64)
    fin = np.isfinite(zd)
    zz = np.where(fin, zd, 0.0)
    d = p[:, :, mcol] - zz
    split, site, time = np.zeros((4, 16)), np.zeros((4, S, 3)), np.zeros((4, nT, 3))
    for c in range(4):
        m = fin & (code == c)
        terms = np.stack([np.where(m, d * d, 0.0), np.where(m, np.abs(d), 0.0), m.astype(np.float64)], axis=2)
        site[c], time[c] = terms.sum(axis=0), terms.sum(axis=1)
        split[c, [1, 2, 0]] = terms.sum(axis=(0, 1))
        for q in range(Q):
            tau = float(np.float32(0.5 if taus is None else taus[q]))
            e = zz - p[:, :, q]
            split[c, 5 + q] = np.where(m, np.maximum((tau - 1.0) * e, tau * e), 0.0).sum()
        if lo >= 0:
            split[c, 3] = (m & (p[:, :, lo] <= zz) & (zz <= p[:, :, hi])).sum()
            split[c, 4] = np.where(m, p[:, :, hi] - p[:, :, lo], 0.0).sum()
    return split, site, time


def close(got, ref, what):
    """1e-12 relative on every value; the counts (slot N, cover, the n of the site / time triples) exact."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref)
    assert np.all(err <= 1e-12 * np.abs(ref)), (what, float((err / np.maximum(np.abs(ref), 1e-300)).max()))
    if got.shape[-1] == 3:
        assert np.array_equal(got[..., 2], ref[..., 2]), what
    else:
        assert np.array_equal(got[:, [0, 3]], ref[:, [0, 3]]), what


def inputs(S, nT, Q, seed):
    rs = np.random.RandomState(seed)
    y = np.sort(rs.standard_normal((nT * S, Q)).astype(np.float32), axis=1)       # levels in order: widths >= 0
    z = rs.standard_normal((nT, S)).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.2] = np.nan
    if S > 3:
        z[:, 3] = np.nan                                                          # a site without a value
    code = rs.randint(0, 4, size=(nT, S)).astype(np.uint8)
    return y, z, code


def run_kernel(y, z, code, mcol, taus, lo, hi, accs=None):
    from stnf import _native as N
    d = T.dev()
    nT, S = z.shape
    if accs is None:
        accs = (torch.zeros(4, N.GRID_SLOTS, dtype=torch.float64, device=d),
                torch.zeros(4, S, 3, dtype=torch.float64, device=d),
                torch.full((4, nT, 3), -7.0, dtype=torch.float64, device=d))      # assigned, not added to
    ws = torch.empty(N.grid_score_workspace_bytes(S, nT) // 8, dtype=torch.float64, device=d)
    N.grid_score(torch.from_numpy(y).to(d), torch.from_numpy(z).to(d),
                 None if code is None else torch.from_numpy(code).to(d), mcol, taus, lo, hi, *accs, ws)
    return accs


@pytest.mark.parametrize("S,nT,Q", [(1, 1, 1), (67, 3, 1), (257, 7, 5), (1031, 2, 8)])
@pytest.mark.parametrize("variant", ["interval", "plain", "no_split"])
def test_kernel_matches_float64(S, nT, Q, variant):
    """One lane; a ragged last wave; more than one workgroup along s (and a second tile group of slices); the widest
    head.  With and without an interval, and with split = NULL."""
    y, z, code = inputs(S, nT, Q, 100 * S + Q)
    taus = TAUS[:Q] if variant != "no_split" else None
    lo, hi = (0, Q - 1) if variant == "interval" and Q > 1 else (-1, -1)
    if variant == "no_split":
        code = None
    got = [a.cpu().numpy() for a in run_kernel(y, z, code, Q // 2, taus, lo, hi)]
    ref = sums64(y, z, np.zeros(z.shape, np.uint8) if code is None else code, Q // 2, taus, lo, hi)
    for g, r, what in zip(got, ref, ("split", "site", "time")):
        close(g, r, (what, S, nT, Q, variant))
    assert got[0][:, 0].sum() == np.isfinite(z).sum()


def test_two_chunks_equal_their_concatenation():
    """site_acc and split_acc add across calls, time_acc is the chunk's own.  A site's slices are added in time order
    either way, so site_acc is bit-equal; split_acc may differ by the order of summation."""
    S, Q = 257, 5
    y, z, code = inputs(S, 20, Q, 9)                    # 17 + 3 slices: the first chunk crosses a tile of 16
    whole = [a.cpu().numpy() for a in run_kernel(y, z, code, 2, TAUS[:Q], 0, 4)]
    first = run_kernel(y[:17 * S], z[:17], code[:17], 2, TAUS[:Q], 0, 4)
    t_first = first[2].cpu().numpy()
    d = T.dev()
    second = run_kernel(y[17 * S:], z[17:], code[17:], 2, TAUS[:Q], 0, 4,
                        accs=(first[0], first[1], torch.zeros(4, 3, 3, dtype=torch.float64, device=d)))
    assert np.array_equal(second[1].cpu().numpy(), whole[1])
    close(second[0].cpu().numpy(), whole[0], "split")
    assert np.array_equal(t_first, whole[2][:, :17]) and np.array_equal(second[2].cpu().numpy(), whole[2][:, 17:])


def test_same_call_same_bits():
    y, z, code = inputs(1031, 5, 3, 21)
    a = [t.cpu().numpy() for t in run_kernel(y, z, code, 1, TAUS[:3], 0, 2)]
    b = [t.cpu().numpy() for t in run_kernel(y, z, code, 1, TAUS[:3], 0, 2)]
    for x, w in zip(a, b):
        assert np.array_equal(x, w)


def grid_model(name):
    if name.endswith("_learn"):
        m = T.build_learn_model(name)[0]
    else:
        m = T.build_model(cases.MODEL_CASES[name])
    if name.startswith("default227"):
        m.force_window_path = False
    return m.eval()


@pytest.mark.parametrize("name", ["c2_b257", "default227", "default227_learn", "c2_b257/dense"])
def test_score_grid_equals_scores_of_predict_grid(name):
    """Window path, materialising path, learnable knots, and the forced materialising forward of the C2 model, whose
    grid goes row by row through predict(); one chunk of 7 slices and chunks of 3 + 3 + 1.  Chunked and
    unchunked predictions are the same bits, so this pins the chunk bookkeeping.  The chunked call never holds the
    grid: after a warm-up call its peak allocation stays below the S*T*Q*4 bytes of the grid alone (so also below the
    grid plus the chunk buffer)."""
    from stnf.engine import Predictor
    S, Tn = 67, 7
    d = T.dev()
    m = grid_model(name.split("/")[0])
    Q = m.output_dim
    rs = np.random.RandomState(5)
    coords = torch.from_numpy(rs.uniform(-0.05, 1.05, (S, 2)).astype(np.float32)).to(d)
    tv = (torch.arange(Tn, dtype=torch.float32) / (Tn - 1)).to(d)
    _, z, code = inputs(S, Tn, Q, 6)
    zt, ct = torch.from_numpy(z).to(d), torch.from_numpy(code).to(d)
    pr = Predictor(m, chunk=32768, force_dense=name.endswith("/dense"))
    for max_rows, slices in ((Tn * S, 7), (3 * S + 5, 3)):
        grid = pr.predict_grid(coords, tv, max_rows=max_rows)
        ref = sums64(grid.reshape(Tn * S, Q).cpu().numpy(), z, code, Q // 2, None, -1, -1)
        pr.score_grid(coords, tv, zt, ct, max_rows=max_rows)                      # warm-up: the predictor's scratch
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        got = pr.score_grid(coords, tv, zt, ct, max_rows=max_rows)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        print(f"{name}: {slices} slices per chunk, peak allocation of the call {peak} B, grid {S * Tn * Q * 4} B, "
              f"buffer {slices * S * Q * 4} B")
        if slices < Tn:
            assert peak < S * Tn * Q * 4 < S * Tn * Q * 4 + slices * S * Q * 4
        for g, r, what in zip(got, ref, ("split", "site", "time")):
            close(g.cpu().numpy(), r, (name, what, slices))


def test_grid_scores_against_evaluator():
    """The test split of grid_scores against Evaluator on the same entries as a DeviceDataset: rows exact; mse and mae
    within what the bound of test_predict_grid_equals_row_by_row on a prediction, delta = 2e-6 max(1, max|y|), does to
    them: |d mse| <= 2 delta mean|err| + delta^2, |d mae| <= delta."""
    from stnf.dataio import DeviceDataset
    from stnf.engine import Predictor
    from stnf.evaluation import Evaluator
    from stnf.utils import grid_scores
    S, Tn = 67, 7
    d = T.dev()
    m = grid_model("c2_b257")
    rs = np.random.RandomState(8)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    _, z, _ = inputs(S, Tn, 1, 9)
    test_mask = rs.uniform(size=z.shape) < 0.3
    got = grid_scores(m, z, coords, test_mask=test_mask)["splits"]
    ds = DeviceDataset.from_mask(z, coords, test_mask)
    ref = Evaluator(m).evaluate(ds, 4096)
    assert got["test"]["rows"] == ref["rows"] == len(ds) > 0
    assert got["all"]["rows"] == int(np.isfinite(z).sum()) and got["train"]["rows"] == got["valid"]["rows"] == 0
    tv = (torch.arange(Tn, dtype=torch.float32) / (Tn - 1)).to(d)
    ymax = Predictor(m).predict_grid(torch.from_numpy(coords).to(d), tv).abs().max().item()
    delta = 2e-6 * max(1.0, ymax)
    print(f"mse {got['test']['mse']!r} vs {ref['mse']!r}, mae {got['test']['mae']!r} vs {ref['mae']!r}, delta {delta}")
    assert abs(got["test"]["mse"] - ref["mse"]) <= 2 * delta * ref["mae"] + delta * delta
    assert abs(got["test"]["mae"] - ref["mae"]) <= delta


@pytest.mark.parametrize("case,word", [("metric_col", "metric_col"), ("lo_ge_hi", "interval"), ("workspace", "workspace")])
def test_kernel_refuses_bad_arguments(case, word):
    from stnf import _native as N
    S, nT, Q = 67, 3, 5
    y, z, code = inputs(S, nT, Q, 1)
    d = T.dev()
    accs = (torch.full((4, N.GRID_SLOTS), 3.0, dtype=torch.float64, device=d),
            torch.full((4, S, 3), 3.0, dtype=torch.float64, device=d),
            torch.full((4, nT, 3), 3.0, dtype=torch.float64, device=d))
    ws = torch.empty(N.grid_score_workspace_bytes(S, nT) // 8, dtype=torch.float64, device=d)
    kw = dict(mcol=Q if case == "metric_col" else 2, lo=3 if case == "lo_ge_hi" else 0, hi=3,
              ws=ws[:-1] if case == "workspace" else ws)
    with pytest.raises(RuntimeError, match=word):
        N.grid_score(torch.from_numpy(y).to(d), torch.from_numpy(z).to(d), torch.from_numpy(code).to(d), kw["mcol"],
                     TAUS[:Q], kw["lo"], kw["hi"], *accs, kw["ws"])
    torch.cuda.synchronize()
    assert all(bool((a == 3.0).all()) for a in accs)           # nothing was launched


def test_score_grid_refuses_covariates():
    from stnf.engine import Predictor
    d = T.dev()
    m = T.build_model(cases.MODEL_CASES["tiny9_ln_p3"]).eval()
    z = torch.zeros(2, 5, device=d)
    with pytest.raises(RuntimeError, match="covariates"):
        Predictor(m).score_grid(torch.rand(5, 2, device=d), torch.tensor([0.0, 1.0], device=d), z)
