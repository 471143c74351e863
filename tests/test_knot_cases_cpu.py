"""The CPU half of the per-knot tests of the learnable-knot gradients (tests/test_gpu_knot_gradients.py):

  * every condition golden/knot_cases.py states about its inputs holds for every case, on the float64 reference alone,
    with no knot and no row left out;
  * the float32 restatement (golden/make_knot_achieved.py) re-run over every case reproduces the committed
    golden/knot_achieved.json, so the recorded K is what this machine measures too;
  * the comparator, at the GPU tests' own K, rejects nine wrong gradients -- each a mutation of the float64 reference
    that touches one knot, one row or one branch and leaves the per-tensor norm within 2e-5 or close to it.
"""
import json

import numpy as np
import pytest

from golden import knot_cases as kc
from golden import make_knot_achieved as mka
from oracle import stdadk_oracle as orc

_CACHE = {}


def _emb(name):
    if name not in _CACHE:
        case = next(c for c in kc.EMB_CASES if c["name"] == name)
        inp = kc.emb_inputs(case)
        _CACHE[name] = (case, inp, kc.emb_eval(case, inp))
    return _CACHE[name]


def _step(name):
    if name not in _CACHE:
        case = next(c for c in kc.STEP_CASES if c["name"] == name)
        inp = kc.step_inputs(case)
        _CACHE[name] = (case, inp, kc.step_data(case, inp))
    return _CACHE[name]


# ------------------------------------------------------------------ conditions
@pytest.mark.parametrize("case", kc.EMB_CASES + kc.MODULE_CASES, ids=lambda c: c["name"])
def test_embedding_case_conditions(case):
    inp = kc.emb_inputs(case)
    ev = kc.emb_eval(case, inp)
    kc.check_conditions(case, inp, ev)
    assert inp["G"].dtype == np.float32 and inp["G"].shape == (case["B"], case["Ks"])
    # support radii spread: with rows at all, a knot that reaches every one of them
    if case["B"] > 0 and case["Ks"] >= 24:
        assert (ev["geo"]["reach"].sum(0) == case["B"]).any()
    # the reference passes its own comparator with nothing to spare
    w = kc.compare_knots(ev["ref"][:, :2], ev["ref"][:, 2], ev)
    assert all(w[k][0] == 0.0 for k in kc.OUTPUTS)


@pytest.mark.parametrize("case", kc.STEP_CASES, ids=lambda c: c["name"])
def test_step_case_conditions(case):
    _, inp, data = _step(case["name"])
    kc.check_conditions(case, inp, data)
    for kt_name in [None] + list(kc.KT_SETTINGS):
        ev = kc.step_eval(data, kt_name)
        kc.compare_knots(ev["ref"][:, :2], ev["ref"][:, 2], ev)
        # an unreached knot under a knot_train: the centre gradient is the penalty term alone
        if kt_name is not None and data["unreached"].any():
            un = data["unreached"]
            kt = kc.KT_SETTINGS[kt_name]
            dc0, _, _ = kc.finish64(np.zeros_like(data["dc"]), np.zeros_like(data["S"]), data["centers"],
                                    data["centers_init"], kt)
            assert np.array_equal(ev["ref"][un, :2], dc0[un]) and np.all(ev["ref"][un, 2] == 0.0)
    # the oracle's G . knot_backward is what learnable_step_grads returned
    p, Ks = inp["cfg"]["p"], len(inp["log_bw"])
    dc, dlb = orc.knot_backward(inp["coords"], inp["centers"], inp["log_bw"], data["dz0"] @ data["W0"][:, p:p + Ks],
                                case["basis"])
    assert np.array_equal(dc, data["dc"]) and np.array_equal(dlb, data["dlb"])


def test_case_tables():
    """The shapes and settings the GPU tests are to run are all there."""
    shapes = {(c["B"], c["Ks"]) for c in kc.EMB_CASES}
    assert {(B, 65) for B in (0, 1, 3, 127, 128, 129, 130, 4096, 4097, 4225)} <= shapes
    assert {(129, Ks) for Ks in (1, 63, 64, 65, 200)} <= shapes and (4225, 200) in shapes
    assert [kc.knot_slabs(B) for B in (1, 128, 129, 4096, 4097, 4225)] == [1, 1, 2, 32, 32, 32]
    assert -(-4097 // 32) == 129 and -(-4225 // 32) == 133
    assert kc.bw_list() >= 8 and kc.bw_list() % 8 == 0
    assert len(kc.DENSE_CASES) == 18 and len(kc.WINDOW_CASES) == 24
    kts = kc.KT_SETTINGS.values()
    assert {k["damping"] for k in kts} == {False, True}
    assert {(k["thr"], k["strength"]) for k in kts if k["damping"]} == {(0.0, 5.0), (0.02, 1.0)}
    assert {k["dom_w"] for k in kts} == {0.0, 0.5} and {k["mov_w"] for k in kts} == {0.0, 0.1}
    assert {k["pgs"] for k in kts} == {1.0, 0.5} and {k["loss"] for k in kts} == {True, False}
    assert abs(kc.sup_prime("wendland") - 2.4998) < 1e-3 
    assert abs(kc.sup_prime("gaussian") - np.exp(-0.5)) < 1e-9 and kc.sup_prime("triangular") == 1.0


# ------------------------------------------------------------------ the recorded K
def test_restatement_reproduces_recorded_figures():
    """Regenerating golden/knot_achieved.json changes nothing beyond what another CPU's float32 exp and GEMM order may
    move (a quarter of the recorded maximum); every case has a record; the bound the GPU tests use follows from it."""
    table = json.load(open(mka.OUT))
    fresh = mka.measure()
    assert set(table["cases"]) == {c["name"] for c in kc.ALL_CASES} == set(fresh["cases"])
    assert table["k_factor"] == kc.K_FACTOR
    for k in kc.OUTPUTS:
        assert fresh["max"][k] <= 1.25 * table["max"][k], (k, fresh["max"][k], table["max"][k])
        assert fresh["max"][k] >= 0.75 * table["max"][k], (k, fresh["max"][k], table["max"][k])
        assert kc.bounds()[k] == kc.K_FACTOR * table["max"][k]
        assert 1.0 <= table["max"][k] <= 32.0, (k, table["max"][k])
    for name, rec in fresh["cases"].items():
        for order, per in rec.items():
            for k, e in per.items():
                assert e <= 1.25 * table["max"][k], (name, order, k, e)


# ------------------------------------------------------------------ mutations the comparator must reject
def _typical_knot(ev, j=0):
    """A reached knot whose |ref| / S is the median of its case: neither the easiest nor the hardest to catch."""
    S, ref = ev["S"][:, j], np.abs(ev["ref"][:, j])
    ks = np.nonzero(S > 0)[0]
    ratio = ref[ks] / S[ks]
    return int(ks[np.argsort(ratio)[len(ks) // 2]])


def _rejected(got, ev):
    with pytest.raises(AssertionError):
        kc.compare_knots(got[:, :2], got[:, 2], ev)


EMB_MUT = ["emb_wendland_B4225_K200", "emb_triangular_B129_K65", "emb_gaussian_B4097_K65"]


@pytest.mark.parametrize("name", EMB_MUT)
def test_rejects_one_row_dropped_from_one_knot(name):
    case, inp, ev = _emb(name)
    geo = ev["geo"]
    k = _typical_knot(ev)
    gr = inp["G"].astype(np.float64)[:, k] * orc.basis_prime(geo["r"][:, k], case["basis"])
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(geo["d"][:, k] > 0, 1.0 / (geo["d"][:, k] * geo["s"][k]), 0.0)
    contrib = np.stack([-gr * geo["dx"][:, k] * inv, -gr * geo["dy"][:, k] * inv, -gr * geo["r"][:, k]], 1)
    assert np.allclose(contrib.sum(0), ev["ref"][k], rtol=1e-9, atol=1e-12)
    rows = np.nonzero(geo["reach"][:, k] & (np.abs(contrib).sum(1) > 0))[0]
    b = rows[np.argsort(np.abs(contrib[rows]).sum(1))[len(rows) // 2]]          # a row of median weight
    got = ev["ref"].copy()
    got[k] -= contrib[b]
    _rejected(got, ev)


@pytest.mark.parametrize("name", EMB_MUT)
def test_rejects_one_knot_scaled_and_axes_swapped(name):
    _, _, ev = _emb(name)
    k = _typical_knot(ev)
    got = ev["ref"].copy()
    got[k] *= 1.0 + 1e-3
    _rejected(got, ev)
    got = ev["ref"].copy()
    got[k, 0], got[k, 1] = ev["ref"][k, 1], ev["ref"][k, 0]
    _rejected(got, ev)


@pytest.mark.parametrize("name", ["emb_wendland_B129_K65", "emb_triangular_B4225_K200"])
def test_rejects_gradient_at_unreached_knot(name):
    _, _, ev = _emb(name)
    k = int(np.nonzero(ev["unreached"])[0][0])
    for j in range(3):
        got = ev["ref"].copy()
        got[k, j] = 1e-12
        _rejected(got, ev)


@pytest.mark.parametrize("name", ["emb_wendland_B129_K65", "emb_gaussian_B4225_K65", "emb_triangular_B129_K200"])
def test_rejects_last_knot_of_ragged_tile_given_its_neighbours_value(name):
    case, _, ev = _emb(name)
    assert case["Ks"] % 64 != 0
    got = ev["ref"].copy()
    got[-1] = ev["ref"][-2]
    _rejected(got, ev)


@pytest.mark.parametrize("name", EMB_MUT)
def test_rejects_bandwidth_gradient_with_the_neighbours_scale(name):
    case, inp, ev = _emb(name)
    k = _typical_knot(ev, 2)
    k = k if k + 1 < case["Ks"] else k - 1
    lb = inp["log_bw"].copy()
    lb[k] = lb[k + 1]
    assert lb[k] != inp["log_bw"][k]
    _, dlb = orc.knot_backward(inp["coords"], inp["centers"], lb, inp["G"], case["basis"])
    got = ev["ref"].copy()
    got[k, 2] = dlb[k]
    _rejected(got, ev)


STEP_MUT = ["dense_wendland_h32_p3_B257", "window_triangular_h128_p0_B1003", "window_wendland_h256_p3_B257"]


@pytest.mark.parametrize("name", STEP_MUT)
@pytest.mark.parametrize("mutate,kt_name", [("lo_sign", "thr0_s5"), ("lo_sign", "damping_off"),
                                            ("damp_first", "thr02_s1_half"), ("damp_first", "no_loss"),
                                            ("no_pgs", "thr02_s1_half"), ("no_pgs", "no_loss")])
def test_rejects_wrong_finish(name, mutate, kt_name):
    """The c < 0 side of the domain penalty with the c > 1 sign; damping before the penalties; pen_grad_scale ignored.
    Each changes a handful of knots."""
    _, _, data = _step(name)
    ev = kc.step_eval(data, kt_name)
    wrong = kc.step_eval(data, kt_name, mutate)["ref"]
    changed = np.nonzero((wrong != ev["ref"]).any(1))[0]
    assert 1 <= len(changed)
    _rejected(wrong, ev)
    if mutate == "lo_sign":
        rel = np.linalg.norm(wrong - ev["ref"]) / np.linalg.norm(ev["ref"])
        print(f"{name} {kt_name} {mutate}: {len(changed)} knots changed, per-tensor rel-L2 {rel:.1e}")


@pytest.mark.parametrize("name", STEP_MUT)
def test_rejects_step_level_single_knot_faults(name):
    """One knot scaled by 1 + 1e-3 and d_cx / d_cy swapped, at step level under a knot_train."""
    _, _, data = _step(name)
    ev = kc.step_eval(data, "thr02_s1_half")
    k = _typical_knot(ev)
    got = ev["ref"].copy()
    got[k] *= 1.0 + 1e-3
    _rejected(got, ev)
    got = ev["ref"].copy()
    got[k, 0], got[k, 1] = ev["ref"][k, 1], ev["ref"][k, 0]
    _rejected(got, ev)
    un = np.nonzero(data["unreached"])[0]
    got = kc.step_eval(data, None)["ref"].copy()
    got[un[0], 2] = 1e-12
    _rejected(got, kc.step_eval(data, None))
