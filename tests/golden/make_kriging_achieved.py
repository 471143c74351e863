"""Measures K_exp, the constant of the device comparison of the exponential and gaussian kriging models
(tests/test_gpu_kriging.py), on the HOST and writes tests/golden/kriging_achieved.json.  Needs no GPU:

    python tests/golden/make_kriging_achieved.py

The device's exp and numpy's may differ in their last bits, so the device's weights differ from
kriging_weights_host's as if every correlation rho had been moved by an ulp or so.  That is emulated here: every rho is
moved by ONE ulp (np.nextafter), up or down by a hash of its own bits and a trial number -- a function of the value, so
that equal distances stay equal, as they do on the device -- and the weights are solved again.  Over TRIALS trials and
every row of kriging_cases.bounded_cases() the worst ratio of |w_perturbed - w| to kappa 2^-52 max|w| is taken (and of
the variance's difference to that times (k + 1) C00), and multiplied by MARGIN = 8: the device's exp is allowed more
than the one ulp emulated (its documented accuracy is 1 ulp, numpy's own below 1 ulp; a few ulp between them leaves a
factor of at least two).  A rho of exactly 0 or 1 stays (exp(-0) and an underflowed exp are exact in both libraries).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "st-dadk_amd")]

from golden import kriging_cases as kc      # noqa: E402
from stnf.utils import kriging as KR        # noqa: E402

TRIALS, MARGIN = 8, 8.0


def perturbed(rho, trial):
    def f(model, d2, range_):
        v = np.asarray(rho(model, d2, range_), dtype=np.float64)
        bits = np.ascontiguousarray(v).view(np.uint64)
        up = ((bits * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03) * np.uint64(trial + 1)) >> np.uint64(63)) == 1
        moved = np.where(up, np.nextafter(v, np.inf), np.nextafter(v, -np.inf))
        return np.where((v == 0.0) | (v == 1.0) | ~np.isfinite(v), v, moved)
    return f


def measure():
    worst_w = worst_v = 0.0
    plain = KR.rho
    for case in kc.bounded_cases():
        tab = kc.table(case)
        args = (tab[0], tab[1], case["k"], case["coords"], case["model"], case["nugget"], case["psill"], case["range"])
        w, var = KR.kriging_weights_host(*args)
        kappa = kc.reference(case, tab)[2]
        scale = kappa * 2.0 ** -52 * np.nan_to_num(np.abs(w).max(axis=2), nan=0.0)
        for trial in range(TRIALS):
            KR.rho = perturbed(plain, trial)
            try:
                w2, var2 = KR.kriging_weights_host(*args)
            finally:
                KR.rho = plain
            assert np.array_equal(np.isnan(w2), np.isnan(w))
            ok = scale > 0
            ew = np.nan_to_num(np.abs(w2 - w).max(axis=2), nan=0.0)
            ev = np.nan_to_num(np.abs(var2 - var), nan=0.0)
            assert (ew[~ok] == 0).all()
            worst_w = max(worst_w, float((ew[ok] / scale[ok]).max(initial=0.0)))
            worst_v = max(worst_v, float((ev[ok] / (scale[ok] * (case["k"] + 1) * (case["nugget"] + case["psill"]))).max(initial=0.0)))
    return worst_w, worst_v


if __name__ == "__main__":
    worst_w, worst_v = measure()
    out = {"trials": TRIALS, "margin": MARGIN, "worst_ratio_w": worst_w, "worst_ratio_var": worst_v,
           "K_exp": MARGIN * max(worst_w, worst_v), "kappa_max": kc.KAPPA_MAX}
    with open(os.path.join(HERE, "kriging_achieved.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)
