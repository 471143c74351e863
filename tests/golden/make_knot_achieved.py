"""Writes tests/golden/knot_achieved.json: what a float32 evaluation of the learnable-knot gradients achieves against
the float64 reference under the bound of knot_cases.compare_knots -- per case of knot_cases, per summation order and
per output, in units of 2^-24 of the output's scale S.

CPU only, numpy only, deterministic:   python tests/golden/make_knot_achieved.py

The GPU tests allow K = knot_cases.K_FACTOR x the maximum recorded here per output (tests/test_gpu_knot_gradients.py);
tests/test_knot_cases_cpu.py re-runs this file's measurement and compares it with the committed JSON.  The measurement
is of this restatement against the float64 reference, never of the library.

What the restatement reproduces: float32 arithmetic throughout -- np.float32 exp of the log-bandwidths, 1 / (bw cal),
the direct distance with np.float32 sqrt, phi' as csrc/knots.hip and csrc/l1_bwd_body.h write it, at step level the
whole forward and backward of the MLP in float32 (the oracle's own functions at dtype float32), the penalties and the
damping factor of knot_finish_kernel -- and the two orders of summation:
  'dense'   G = dZ0 . W0 first; then per knot the rows of a slab on four interleaved chains, the slabs on four
            interleaved chains (knot_grad_kernel, knot_finish_kernel);
  'window'  per knot sum_b q_b dZ0[b, :] over the rows with phi != 0 in the order of the binning, one chain per hidden
            unit, then the dot product with the knot's column of W0 (l1_window_bwd_body, KNOTS = true).
What it does not: fused multiply-adds, the GPU's division, expf and square root, the order inside a GEMM -- the factor
of 4 is for those.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from golden import knot_cases as kc                       # noqa: E402
from golden import site_cases as sc                       # noqa: E402
from oracle import stdadk_oracle as orc                   # noqa: E402

OUT = kc.ACHIEVED
F = np.float32


def prime32(r, basis):
    one = F(1.0)
    if basis == "wendland":
        om = one - r
        om2 = om * om
        v = (F(-56.0) / F(3.0)) * r * (om2 * om2 * om) * (F(5.0) * r + one)
        return np.where(r < one, v, F(0.0)).astype(F)
    if basis == "gaussian":
        return (-r * np.exp(F(-0.5) * r * r)).astype(F)
    return np.where(r <= one, F(-1.0), F(0.0)).astype(F)


def phi32(r, basis):
    one = F(1.0)
    if basis == "wendland":
        r = np.minimum(r, one)
        om = one - r
        om2 = om * om
        return (om2 * om2 * om2) * ((F(35.0) * r + F(18.0)) * r + F(3.0)) * (one / F(3.0))
    if basis == "gaussian":
        return np.exp(F(-0.5) * r * r)
    return np.maximum(one - r, F(0.0))


def pair_factors32(coords, centers, log_bw, basis):
    """Per (row, knot), float32: inv_s, d, r, phi'(r), dx, dy, phi."""
    x, c = np.asarray(coords, F).reshape(-1, 2), np.asarray(centers, F)
    inv_s = F(1.0) / (np.exp(np.asarray(log_bw, F)) * F(orc.CALIBRATION_FACTORS[basis]))
    dx = x[:, 0:1] - c[None, :, 0]
    dy = x[:, 1:2] - c[None, :, 1]
    d = np.sqrt(dx * dx + dy * dy)
    r = d * inv_s[None, :]
    out = dict(inv_s=inv_s, dx=dx, dy=dy, d=d, r=r, gp=prime32(r, basis), phi=phi32(r, basis))
    assert all(a.dtype == F for a in out.values())
    return out


def _chain(A):
    """One float32 chain down axis 0 (cumsum adds in order; sum would add pairwise)."""
    if A.shape[0] == 0:
        return np.zeros(A.shape[1:], dtype=F)
    return np.cumsum(A, axis=0, dtype=F)[-1]


def slab_sum32(C):
    """(B, Ks) float32 contributions -> (Ks,) in the order of knot_grad_kernel + knot_finish_kernel."""
    B = C.shape[0]
    if B == 0:
        return np.zeros(C.shape[1], dtype=F)
    slabs = kc.knot_slabs(B)
    rows_per = -(-B // slabs)
    parts = np.zeros((slabs, C.shape[1]), dtype=F)
    for s in range(slabs):
        r0, r1 = s * rows_per, min(B, (s + 1) * rows_per)
        w = [_chain(C[r0 + i:r1:4]) if r0 + i < r1 else np.zeros(C.shape[1], dtype=F) for i in range(4)]
        parts[s] = (w[0] + w[1]) + (w[2] + w[3])
    w = [_chain(parts[i::4]) for i in range(4)]
    return (w[0] + w[1]) + (w[2] + w[3])


def dense32(G, pf):
    """The three raw sums (Ks, 3) float32 of the materialising route from G (B, Ks) float32."""
    gr = G * pf["gp"]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(pf["d"] > 0, gr * pf["inv_s"][None, :] / pf["d"], F(0.0)).astype(F)
    return np.stack([slab_sum32(-q * pf["dx"]), slab_sum32(-q * pf["dy"]), slab_sum32(-gr * pf["r"])], axis=1)


def window32(dz0, W0k, pf, order):
    """The three raw sums (Ks, 3) float32 of the window route: dz0 (B, H), W0k (H, Ks) the knots' columns of W0, rows
    visited in `order` (the binning's)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        qd = np.where(pf["d"] > 0, pf["gp"] * pf["inv_s"][None, :] / pf["d"], F(0.0)).astype(F)
    q = (-qd * pf["dx"], -qd * pf["dy"], -pf["gp"] * pf["r"])
    Ks = W0k.shape[1]
    out = np.zeros((Ks, 3), dtype=F)
    for k in range(Ks):
        rows = order[pf["phi"][order, k] != 0]
        if rows.size == 0:
            continue
        for j in range(3):
            acc = _chain(q[j][rows, k][:, None] * dz0[rows])                  # (H,) one chain per hidden unit
            out[k, j] = np.sum(acc * W0k[:, k], dtype=F)
    return out


def finish32(raw, centers, centers_init, kt):
    """knot_finish_kernel after the slab sums, in float32: (d_centers (Ks, 2), d_log_bw (Ks,))."""
    gx, gy, gl = raw[:, 0].copy(), raw[:, 1].copy(), raw[:, 2].copy()
    if kt is not None:
        c, ci = np.asarray(centers, F), np.asarray(centers_init, F)
        cx, cy = c[:, 0], c[:, 1]
        mx, my = cx - ci[:, 0], cy - ci[:, 1]
        dom_w, mov_w, pgs, zero, one, two = F(kt["dom_w"]), F(kt["mov_w"]), F(kt["pgs"]), F(0.0), F(1.0), F(2.0)
        if dom_w > 0:
            for cc, tgt in ((cx, "x"), (cy, "y")):
                v = np.maximum(zero - cc, zero) + np.maximum(cc - one, zero)
                sg = np.where(cc > one, one, np.where(cc < zero, -one, zero)).astype(F)
                add = (pgs * dom_w) * (two * v * sg)
                if tgt == "x":
                    gx = gx + add
                else:
                    gy = gy + add
        if mov_w > 0:
            gx = gx + (pgs * mov_w) * (two * mx)
            gy = gy + (pgs * mov_w) * (two * my)
        if kt["damping"]:
            dist = np.sqrt(mx * mx + my * my)
            f = np.exp(-F(kt["strength"]) * np.maximum(dist - F(kt["thr"]), zero))
            gx, gy = gx * f, gy * f
    out = np.stack([gx, gy], axis=1), gl
    assert out[0].dtype == F and out[1].dtype == F
    return out


def _merge(into, worst):
    for k in kc.OUTPUTS:
        into[k] = max(into.get(k, 0.0), round(worst[k][0], 3))


def measure_emb(case):
    inp = kc.emb_inputs(case)
    ev = kc.emb_eval(case, inp)
    pf = pair_factors32(inp["coords"], inp["centers"], inp["log_bw"], case["basis"])
    dc, dlb = finish32(dense32(inp["G"], pf), inp["centers"], None, None)
    inf = {k: float("inf") for k in kc.OUTPUTS}
    out = {}
    _merge(out, kc.compare_knots(dc, dlb, ev, K=inf))
    return {"dense": out}


def measure_step(case):
    inp = kc.step_inputs(case)
    data = kc.step_data(case, inp)
    cfg = inp["cfg"]
    p, Ks = cfg["p"], len(inp["log_bw"])
    _, dz0, W0 = kc.step_pass(inp, np.float32)
    assert dz0.dtype == F and W0.dtype == F
    W0k = np.ascontiguousarray(W0[:, p:p + Ks])
    pf = pair_factors32(inp["coords"], inp["centers"], inp["log_bw"], case["basis"])
    raws = {"dense": dense32((dz0 @ W0k).astype(F), pf)}
    if case["basis"] in kc.COMPACT:
        order = np.argsort(orc.cell_keys(inp["coords"], sc.pick_cell_grid(case["B"])), kind="stable")
        raws["window"] = window32(dz0, W0k, pf, order)
    inf = {k: float("inf") for k in kc.OUTPUTS}
    out = {}
    for name, raw in raws.items():
        out[name] = {}
        for kt_name in [None] + list(kc.KT_SETTINGS):
            kt = kc.KT_SETTINGS[kt_name] if kt_name else None
            dc, dlb = finish32(raw, inp["centers"], inp["centers_init"], kt)
            _merge(out[name], kc.compare_knots(dc, dlb, kc.step_eval(data, kt_name), K=inf))
    return out


def measure(progress=False):
    cases_out, worst = {}, {k: 0.0 for k in kc.OUTPUTS}
    for case in kc.ALL_CASES:
        rec = measure_emb(case) if case["level"] == "emb" else measure_step(case)
        cases_out[case["name"]] = rec
        for per in rec.values():
            for k, e in per.items():
                worst[k] = max(worst[k], e)
        if progress:
            print(case["name"], rec, flush=True)
    return dict(unit="2^-24 of S (knot_cases.compare_knots)", k_factor=kc.K_FACTOR, max=worst, cases=cases_out)


def main():
    table = measure(progress="-v" in sys.argv)
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, "max:", table["max"])


if __name__ == "__main__":
    main()
