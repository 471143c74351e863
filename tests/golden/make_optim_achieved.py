"""Writes tests/golden/optim_achieved.json: what a float32 evaluation of one clip + AdamW + EMA step, in the order of
operations of csrc/optim.hip, achieves against the float64 reference (oracle.adamw_ema_elementwise) under the bound of
optim_cases.normalised_errors -- per case of optim_cases and per output, in units of 2^-24 of the output's scale.

CPU only, numpy only, deterministic:   python tests/golden/make_optim_achieved.py

The GPU tests allow K = optim_cases.K_FACTOR x the maximum recorded here per output (tests/test_gpu_optim_elementwise.py);
tests/test_optim_elementwise_cpu.py re-runs this file's measurement and compares it with the committed JSON.

What the restatement reproduces: every rounding of adam_one and of the launch's prologue (clip coefficient from
the float32 sum of the partials, bias corrections from a power rounded to float32, 1 / sqrt(bc2), lr / bc1, 1 - lr wd).  What it
does not: fused multiply-adds (each is a product and a sum rounded separately here), the GPU's division, square root
and powf -- the factor of 4 is for those.

`tiny_sv_share`: the share of elements with 0 < S_v < 1e-30, where (1 - b2) g'^2 would be near float32's subnormals
and an ulp of v' no longer a relative quantity.  It must be 0 (asserted): the inputs keep |g| >= 1e-12 or exactly 0.
(Elements with S_v == 0 -- a zero gradient on zero moments -- are not in that share: they must match exactly.)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from golden import optim_cases as oc                      # noqa: E402
from oracle import stdadk_oracle as orc                   # noqa: E402

OUT = os.path.join(HERE, "optim_achieved.json")
F = np.float32
OUTPUTS = ("p", "m", "v", "ema")


def sumsq_parts_f32(g, parts=256):
    """Partials as the sumsq launch leaves them, up to the order inside a partial: the sum of squares of every
    `parts`-th slice, rounded to float32."""
    g = np.asarray(g, dtype=np.float64)
    return np.array([(g[b::parts] ** 2).sum() for b in range(parts)]).astype(F)


def _sum_parts_f32(parts):
    """256 chains over the partials (thread t takes t, t + 256, ...), then a pairwise tree, all in float32."""
    pad = np.zeros(-(-parts.size // 256) * 256, dtype=F)
    pad[:parts.size] = parts
    acc = np.zeros(256, dtype=F)
    for row in pad.reshape(-1, 256):
        acc = acc + row
    while acc.size > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def step_f32(inp, case, parts):
    """The step in float32, rounding where the kernel rounds.  Returns {p, m, v, ema} (float32)."""
    h = oc.case_hyper(case)
    lr, b1, b2, eps, wd = F(h["lr"]), F(h["betas"][0]), F(h["betas"][1]), F(h["eps"]), F(h["weight_decay"])
    d, gmul, one = F(h["ema_decay"]), F(case["grad_mul"]), F(1.0)
    coef = one
    if case["clip"] is not None:
        ss = _sum_parts_f32(parts)
        coef = np.minimum(one, F(h["max_norm"]) / (np.sqrt(ss) + F(1e-6)))
    gm = coef * gmul
    # (the correctly rounded float32 power: numpy's own float32 power differs in the last bit between CPUs, and the
    #  recorded figures must not; C_POW allows the GPU's powf its ulps)
    bc1 = one - F(float(b1) ** case["step"])
    bc2 = one - F(float(b2) ** case["step"])
    step_size = lr / bc1
    inv_sqrt_bc2 = one / np.sqrt(bc2)
    decay_mul = one - lr * wd
    g = inp["g"] * gm
    p = inp["p"] * decay_mul
    m = b1 * inp["m"] + (one - b1) * g
    v = b2 * inp["v"] + ((one - b2) * g) * g
    denom = np.sqrt(v) * inv_sqrt_bc2 + eps
    p = p - step_size * (m / denom)
    out = dict(p=p, m=m, v=v, ema=None)
    if inp["ema"] is not None:
        out["ema"] = d * inp["ema"] + (one - d) * p
    assert all(a is None or a.dtype == F for a in out.values())
    return out


def reference(inp, case, parts):
    """The float64 reference of the case (oracle.adamw_ema_elementwise) with the clip coefficient from `parts`."""
    h = oc.case_hyper(case)
    coef = oc.clip_coef64(parts, h["max_norm"]) if case["clip"] is not None else 1.0
    return orc.adamw_ema_elementwise(inp["p"], inp["g"], inp["m"], inp["v"], inp["ema"], case["step"], h["lr"],
                                     h["betas"], h["eps"], h["weight_decay"], coef, case["grad_mul"], h["ema_decay"])


def all_cases():
    return oc.ADAMW_CASES + [oc.adamw2_group_case(c2, i) for c2 in oc.ADAMW2_CASES for i in range(2)]


def measure_case(case):
    """({output: ulps}, share of 0 < S_v < 1e-30) of one case; asserts exactness wherever a scale is 0."""
    inp = oc.make_inputs(case)
    parts = sumsq_parts_f32(inp["g"]) if case["clip"] == "sumsq" else inp["parts"]
    ref = reference(inp, case, parts)
    h = oc.case_hyper(case)
    errs = oc.normalised_errors(step_f32(inp, case, parts), ref, h["betas"], case["step"], h["ema_decay"])
    for k, (_, exact) in errs.items():
        assert exact, (case["name"], k, "differs from the reference where its scale is 0")
    share = float(np.mean((ref["S_v"] > 0) & (ref["S_v"] < 1e-30)))
    assert share == 0.0, (case["name"], share)
    return {k: e for k, (e, _) in errs.items()}, share


def measure():
    cases_out, worst = {}, {k: 0.0 for k in OUTPUTS}
    for case in all_cases():
        errs, share = measure_case(case)
        cases_out[case["name"]] = dict({k: round(e, 3) for k, e in errs.items()}, tiny_sv_share=share)
        for k, e in errs.items():
            worst[k] = max(worst[k], round(e, 3))
    return dict(unit="2^-24 of S (optim_cases.normalised_errors)", c_pow=oc.C_POW, max=worst, cases=cases_out)


def main():
    table = measure()
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, "max:", table["max"])


if __name__ == "__main__":
    main()
