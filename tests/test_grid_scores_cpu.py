"""Grid scores without a GPU: the host path of stnf.utils.predictions.grid_scores against a numpy float64 restatement
written here, against evaluate_model per split, its T == 1 and overlapping-mask rules, the npz record, and the ABI of
stdadk_grid_score_f32 (header, binding and library; its argument checks run in a child process under STDADK_DRY_RUN=1,
where the library validates and launches nothing)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, T = 37, 4
TAUS5 = [0.05, 0.25, 0.5, 0.75, 0.95]


def build(name):
    from stnf.models import STInterpMLP
    if name in cases.QUANTILE_CASES:
        cfg, loss = cases.quantile_cfg(name)
        config = {"regression_type": "multi-quantile", "quantile_levels": list(loss["taus"])}
    else:
        cfg, config = cases.MODEL_CASES[name], {"regression_type": "mean"}
    m = STInterpMLP(p=cfg["p"], k_spatial_centers=cfg["k_spatial_centers"], k_temporal_centers=cfg["k_temporal_centers"],
                    hidden_dims=cfg["hidden_dims"], dropout=0.0, layernorm=cfg["layernorm"],
                    spatial_basis_function=cfg["basis"], output_dim=cfg["output_dim"])
    st = cases.make_state(cfg)
    with torch.no_grad():
        for (_, p), (k, v) in zip(m.named_parameters(), st.items()):
            assert tuple(p.shape) == v.shape, k
            p.copy_(torch.from_numpy(v.copy()))
    return m.eval(), config


def field(seed, n_t=T):
    """coords, z (about 20 % NaN, site 5 and time 2 all NaN) and three disjoint masks that leave entries in none."""
    rs = np.random.RandomState(seed)
    coords = rs.uniform(0, 1, (S, 2)).astype(np.float32)
    z = rs.standard_normal((n_t, S)).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.2] = np.nan
    z[:, 5] = np.nan
    if n_t > 2:
        z[2, :] = np.nan
    u = rs.uniform(size=z.shape)
    return coords, z, u < 0.4, (u >= 0.4) & (u < 0.6), (u >= 0.6) & (u < 0.85)


def model_grid(m, coords, n_t):
    """(T, S, Q) float64: the model's own predictions, time slice by time slice."""
    c = torch.from_numpy(coords)
    with torch.no_grad():
        return np.stack([m(torch.zeros(S, 0), c, torch.full((S, 1), float(np.float32(i) / np.float32(n_t - 1)) if n_t > 1
                                                            else 0.0)).double().numpy() for i in range(n_t)])


def nanratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b > 0, a / np.where(b > 0, b, 1), np.nan)


def oracle(pred, z, code, levels=None, interval=None):
    """The scores in float64 numpy, from the definitions."""
    Tn, Sn, Q = pred.shape
    z = z.astype(np.float64)
    fin = np.isfinite(z)
    err = pred[:, :, Q // 2] - z
    out = {"splits": {}}
    sel = {"all": fin, "other": fin & (code == 0), "train": fin & (code == 1), "valid": fin & (code == 2),
           "test": fin & (code == 3)}
    for name, m in sel.items():
        n = int(m.sum())
        d = {"rows": n, "mse": float(np.mean(err[m] ** 2)) if n else np.nan,
             "mae": float(np.mean(np.abs(err[m]))) if n else np.nan}
        d["rmse"] = d["mse"] ** 0.5
        if levels is not None:
            ck = []
            for q, tau in enumerate(levels):
                e = (z - pred[:, :, q])[m]
                ck.append(float(np.mean(np.maximum((tau - 1) * e, tau * e))) if n else np.nan)
            if len(levels) == 1:
                d["check_loss"] = ck[0]
            else:
                d["mean_check_loss"] = d["check_loss"] = float(np.mean(ck))
                d["crps"] = 2.0 * float(np.mean(ck))
        if interval is not None:
            lo, hi = levels.index(interval[0]), levels.index(interval[1])
            d["coverage"] = float(np.mean((pred[:, :, lo] <= z)[m] & (z <= pred[:, :, hi])[m])) if n else np.nan
            d["mean_width"] = float(np.mean((pred[:, :, hi] - pred[:, :, lo])[m])) if n else np.nan
        out["splits"][name] = d
    e2, e1 = np.where(fin, err ** 2, 0.0), np.where(fin, np.abs(err), 0.0)
    for name, ax in (("site", 0), ("time", 1)):
        cnt = fin.sum(axis=ax)
        out[f"{name}_mse"], out[f"{name}_mae"] = nanratio(e2.sum(axis=ax), cnt), nanratio(e1.sum(axis=ax), cnt)
        out[f"{name}_count"] = cnt
        out[f"{name}_mse_by_split"] = np.stack([nanratio(np.where(fin & (code == c), e2, 0.0).sum(axis=ax),
                                                         (fin & (code == c)).sum(axis=ax)) for c in range(4)])
    return out


def assert_scores(got, ref, rtol):
    assert set(got) == set(ref)
    for name, d in ref["splits"].items():
        assert set(got["splits"][name]) == set(d), name
        for k, v in d.items():
            g = got["splits"][name][k]
            if k == "rows":
                assert g == v, (name, k, g, v)
            else:
                assert (np.isnan(v) and np.isnan(g)) or abs(g - v) <= rtol * abs(v), (name, k, g, v)
    for k, v in ref.items():
        if k == "splits":
            continue
        g = np.asarray(got[k])
        assert g.shape == v.shape, k
        if k.endswith("_count"):
            assert np.array_equal(g, v), k
        else:
            assert np.array_equal(np.isnan(g), np.isnan(v)), k
            ok = ~np.isnan(v)
            assert np.all(np.abs(g[ok] - v[ok]) <= rtol * np.abs(v[ok])), (k, np.abs(g[ok] - v[ok]).max())


def codes(tr, va, te):
    code = np.zeros(tr.shape, dtype=np.uint8)
    code[tr], code[va], code[te] = 1, 2, 3
    return code


@pytest.mark.parametrize("name", ["tiny9", "tiny9_mq5_nc1"])
def test_host_path_matches_float64_oracle(name):
    from stnf.utils import grid_scores
    m, config = build(name)
    coords, z, tr, va, te = field(3)
    levels = config.get("quantile_levels")
    interval = None
    if levels is not None:
        interval = (levels[0], levels[-1])
        config = dict(config, interval=interval)
    got = grid_scores(m, z, coords, tr, va, te, config)
    ref = oracle(model_grid(m, coords, T), z, codes(tr, va, te), levels, interval)
    assert_scores(got, ref, 1e-12)
    assert np.isnan(got["site_mse"][5]) and got["site_count"][5] == 0
    assert np.isnan(got["time_mse"][2]) and got["time_count"][2] == 0
    assert got["splits"]["other"]["rows"] > 0
    assert got["splits"]["all"]["rows"] == sum(got["splits"][k]["rows"] for k in ("train", "valid", "test", "other"))


@pytest.mark.parametrize("name", ["tiny9", "tiny9_mq5_nc1"])
def test_split_metrics_match_evaluate_model(name):
    """evaluate_model works in float32 numpy over at most 150 rows: a few 2^-24 of error, 1e-5 is the margin."""
    from stnf.dataio import DeviceDataset
    from stnf.utils import grid_scores
    from stnf.utils.predictions import evaluate_model
    m, config = build(name)
    coords, z, tr, va, te = field(4)
    got = grid_scores(m, z, coords, tr, va, te, config)
    for split, mask in (("train", tr), ("valid", va), ("test", te)):
        ds = DeviceDataset.from_mask(z, coords, mask, device="cpu")
        ref = evaluate_model(m, ds, config)
        assert got["splits"][split]["rows"] == len(ds) > 0
        assert set(ref) <= set(got["splits"][split])
        for k, v in ref.items():
            assert abs(got["splits"][split][k] - v) <= 1e-5 * abs(v), (split, k, got["splits"][split][k], v)


def test_single_time_uses_t_zero():
    from stnf.utils import grid_scores
    m, config = build("tiny9")
    coords, z, tr, va, te = field(5, n_t=1)
    got = grid_scores(m, z, coords, tr, va, te, config)
    with torch.no_grad():
        pred = m(torch.zeros(S, 0), torch.from_numpy(coords), torch.zeros(S, 1)).double().numpy()[None]
    assert_scores(got, oracle(pred, z, codes(tr, va, te)), 1e-12)
    assert got["time_mse"].shape == (1,) and got["site_mse"].shape == (S,)


def test_overlapping_masks_resolve_to_the_higher_code():
    from stnf.utils import grid_scores
    m, config = build("tiny9")
    coords, z, tr, va, te = field(6)
    tr2, va2 = tr | va | te, va | te                  # every test entry is in all three masks, every valid one in two
    got = grid_scores(m, z, coords, tr2, va2, te, config)
    ref = grid_scores(m, z, coords, tr, va, te, config)
    assert_scores(got, oracle(model_grid(m, coords, T), z, codes(tr, va, te)), 1e-12)
    assert got["splits"]["test"] == ref["splits"]["test"] and got["splits"]["train"] == ref["splits"]["train"]


def test_save_grid_scores_npz_round_trips(tmp_path):
    from stnf.utils import grid_scores, save_grid_scores_npz
    m, config = build("tiny9_mq5_nc1")
    coords, z, tr, va, te = field(7)
    got = grid_scores(m, z, coords, tr, va, te, config)
    path = save_grid_scores_npz(tmp_path / "out", got)
    assert os.path.basename(path) == "grid_scores.npz"
    back = np.load(path)
    for k, v in got.items():
        if k != "splits":
            assert np.array_equal(back[k], v, equal_nan=True), k
    for split, d in got["splits"].items():
        for k, v in d.items():
            assert np.array_equal(back[f"splits/{split}/{k}"], np.asarray(v), equal_nan=True), (split, k)


# ---- ABI ------------------------------------------------------------------------------------------------------
C_TYPES = {"const float *": ctypes.c_void_p, "const uint8_t *": ctypes.c_void_p, "double *": ctypes.c_void_p,
           "void *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t,
           "stdadk_stream_t": ctypes.c_void_p}


def test_abi_10_header_binding_and_library_agree():
    from stnf import _native as N
    hdr = open(os.path.join(ROOT, "include", "stdadk.h")).read()
    assert int(re.search(r"#define\s+STDADK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == N.ABI_VERSION
    assert N.lib().stdadk_abi_version() == 10
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, res in (("stdadk_grid_score_f32", ctypes.c_int), ("stdadk_grid_score_workspace_bytes", ctypes.c_size_t)):
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % sym, code, flags=re.S).group(1)
        want = []
        for a in args.split(","):
            ctype = re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()
            want.append(C_TYPES[ctype])
        got_res, got_args = N._SIGNATURES[sym]
        assert got_res is res
        # the host array of levels is the one typed pointer of the binding
        assert [ctypes.c_void_p if a is ctypes.POINTER(ctypes.c_float) else a for a in got_args] == want, sym
        assert hasattr(ctypes.CDLL(N.LIB_PATH), sym)
    for name in ("N", "SSE", "SAE", "COVER", "WIDTH", "CHECK", "SLOTS"):
        assert int(re.search(r"#define\s+STDADK_GRID_%s\s+(\d+)" % name, hdr).group(1)) == getattr(N, "GRID_" + name)


def drive():
    """Child process under STDADK_DRY_RUN=1: return codes and messages of the entry's argument checks."""
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    from stnf import _native as N
    Sn, nT, Q = 67, 3, 5
    y, z = torch.zeros(nT * Sn, Q), torch.zeros(nT, Sn)
    sp = torch.zeros(nT, Sn, dtype=torch.uint8)
    accs = lambda: (torch.zeros(4, N.GRID_SLOTS, dtype=torch.float64), torch.zeros(4, Sn, 3, dtype=torch.float64),
                    torch.zeros(4, nT, 3, dtype=torch.float64))
    need = N.grid_score_workspace_bytes(Sn, nT)
    ws = torch.zeros(need // 8, dtype=torch.float64)
    rec = {"need": need}

    def call(key, **kw):
        a = dict(y=y, z=z, split=sp, mcol=Q // 2, taus=TAUS5, lo=0, hi=4, ws=ws)
        a.update(kw)
        try:
            N.grid_score(a["y"], a["z"], a["split"], a["mcol"], a["taus"], a["lo"], a["hi"], *accs(), a["ws"])
            rec[key] = None
        except RuntimeError as e:
            rec[key] = str(e)
    call("good")
    call("no_split_no_interval", split=None, taus=None, lo=-1, hi=-1)
    call("metric_col", mcol=Q)
    call("lo_ge_hi", lo=3, hi=3)
    call("half_interval", lo=-1, hi=2)
    call("workspace", ws=ws[:-1])
    try:
        N.grid_score_workspace_bytes(1 << 16, 1 << 15)
        rec["too_large"] = None
    except RuntimeError as e:
        rec["too_large"] = str(e)
    print("RECORD " + json.dumps(rec))


@pytest.fixture(scope="module")
def rec():
    env = dict(os.environ, STDADK_DRY_RUN="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RECORD ")][-1]
    return json.loads(line[len("RECORD "):])


def test_entry_accepts_good_arguments(rec):
    assert rec["good"] is None and rec["no_split_no_interval"] is None
    assert rec["need"] == 8 * (1 * 3 * 12 + 4 * 10)          # one workgroup of sites: 12 values per slice + 4 x 10


@pytest.mark.parametrize("case,word", [("metric_col", "metric_col"), ("lo_ge_hi", "interval"), ("half_interval", "interval"),
                                       ("workspace", "workspace"), ("too_large", "2^31")])
def test_entry_refuses_bad_arguments(rec, case, word):
    assert rec[case] is not None and word in rec[case], rec[case]


if __name__ == "__main__":
    drive()
