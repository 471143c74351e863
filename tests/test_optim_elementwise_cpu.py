"""CPU half of the per-element optimiser tests (the GPU half: test_gpu_optim_elementwise.py).

  * oracle.adamw_ema_elementwise, the float64 reference with per-element error scales, against adamw_ema_step and
    against torch.optim.AdamW + clip_grad_norm_ in float64, to 1e-12;
  * the float32 restatement of csrc/optim.hip's order of operations (golden/make_optim_achieved.py) re-run over every
    case of golden/optim_cases.py: it reproduces the committed golden/optim_achieved.json, and so stays inside the
    bound  |got - ref| <= K 2^-24 S + A  with K = the recorded maximum -- the GPU tests' K without its factor of 4.
"""
import json
import math

import numpy as np
import torch

from golden import make_optim_achieved as moa
from golden import optim_cases as oc
from oracle import stdadk_oracle as orc

F32 = lambda x: float(np.float32(x))                                                    # noqa: E731


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b))), (what, float(np.abs(a - b).max()))


def _hyper32(h):
    return dict(lr=F32(h["lr"]), betas=(F32(h["betas"][0]), F32(h["betas"][1])), eps=F32(h["eps"]),
                weight_decay=F32(h["weight_decay"]), ema_decay=F32(h["ema_decay"]), max_norm=F32(h["max_norm"]))


def _case(step, hyper):
    return dict(name=f"cpu_{hyper}_{step}", n=1027, step=step, hyper=hyper, ema=True, clip=None)


def test_elementwise_matches_adamw_ema_step():
    """Same step, two statements of it: the dict-of-arrays oracle the goldens pin and the flat one with scales.  The
    hyper-parameters go to adamw_ema_step already rounded to float32, which is what the flat one does to them."""
    for hyper in oc.HYPER:
        for step in oc.STEPS:
            inp = oc.make_inputs(_case(step, hyper))
            h = _hyper32(oc.HYPER[hyper])
            for max_norm in (0.0, h["max_norm"]):
                d = {k: {"w": inp[k].astype(np.float64).copy()} for k in ("p", "g", "m", "v", "ema")}
                coef = orc.adamw_ema_step(d["p"], d["g"], d["m"], d["v"], d["ema"], step, h["lr"], h["weight_decay"],
                                          h["betas"], h["eps"], max_norm, h["ema_decay"])
                assert (coef < 1.0) == (max_norm > 0)
                r = orc.adamw_ema_elementwise(inp["p"], inp["g"], inp["m"], inp["v"], inp["ema"], step,
                                              oc.HYPER[hyper]["lr"], oc.HYPER[hyper]["betas"], oc.HYPER[hyper]["eps"],
                                              oc.HYPER[hyper]["weight_decay"], coef, 1.0, oc.HYPER[hyper]["ema_decay"])
                for k in ("p", "m", "v", "ema"):
                    _close(r[k], d[k]["w"], (hyper, step, max_norm, k))
                for k in ("S_p", "S_m", "S_v", "S_e"):
                    assert np.all(r[k] >= 0) and np.all(np.isfinite(r[k]))
                _close(r["p"], inp["p"].astype(np.float64) * (1.0 - h["lr"] * h["weight_decay"]) - r["U"], "U")


def test_elementwise_matches_torch_adamw_in_float64():
    """torch.optim.AdamW + clip_grad_norm_ on float64 tensors, three consecutive steps (torch keeps the moments and
    the step count itself), grad_mul applied to the clipped gradient, the EMA as stnf/utils/ema.py forms it."""
    for hyper in oc.HYPER:
        h = _hyper32(oc.HYPER[hyper])
        inp = oc.make_inputs(_case(1, hyper))
        p = torch.nn.Parameter(torch.from_numpy(inp["p"].astype(np.float64)))
        opt = torch.optim.AdamW([p], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"],
                                foreach=False)
        ema_t = torch.from_numpy(inp["ema"].astype(np.float64))
        cur = {k: inp[k].astype(np.float64) for k in ("p", "m", "v", "ema")}
        for step, grad_mul in ((1, 1.0), (2, 0.25), (3, 1.0)):
            g = oc.make_inputs(_case(step + 100, hyper))["g"].astype(np.float64)
            p.grad = torch.from_numpy(g.copy())
            total = torch.nn.utils.clip_grad_norm_([p], h["max_norm"])
            coef = min(1.0, h["max_norm"] / (float(total) + 1e-6))
            assert coef < 1.0
            p.grad.mul_(grad_mul)
            opt.step()
            ema_t = h["ema_decay"] * ema_t + (1.0 - h["ema_decay"]) * p.detach()
            r = orc.adamw_ema_elementwise(cur["p"], g, cur["m"], cur["v"], cur["ema"], step, h["lr"], h["betas"],
                                          h["eps"], h["weight_decay"], coef, grad_mul, h["ema_decay"])
            st = opt.state[p]
            _close(r["p"], p.detach().numpy(), (hyper, step, "p"))
            _close(r["m"], st["exp_avg"].numpy(), (hyper, step, "m"))
            _close(r["v"], st["exp_avg_sq"].numpy(), (hyper, step, "v"))
            _close(r["ema"], ema_t.numpy(), (hyper, step, "ema"))
            cur = {k: r[k] for k in ("p", "m", "v", "ema")}


def test_hyper_parameters_are_rounded_to_float32_first():
    """1 - float32(0.999) is 1.3e-5 away from 1 - 0.999: a reference that keeps the doubles is hundreds of fp32 ulps
    from what any fp32 kernel can compute at step 1."""
    inp = oc.make_inputs(_case(1, "opt"))
    h = oc.HYPER["opt"]
    r = orc.adamw_ema_elementwise(inp["p"], inp["g"], inp["m"], inp["v"], None, 1, h["lr"], h["betas"], h["eps"],
                                  h["weight_decay"], 1.0, 1.0, 0.0)
    assert r["ema"] is None and r["S_e"] is None
    g = inp["g"].astype(np.float64)
    v_doubles = (1.0 - h["betas"][1]) * g * g
    nz = g != 0
    rel = np.abs(r["v"][nz] - v_doubles[nz]) / r["v"][nz]
    assert 1e-5 < rel.min() and rel.max() < 2e-5
    _close(r["v"], (1.0 - F32(h["betas"][1])) * g * g, "v")


def test_absolute_term_is_what_the_bias_corrections_cost():
    """A_p = c_pow 2^-24 (b1^t / bc1 + b2^t / (2 bc2)) |U|: large at the first steps, nothing at large ones."""
    for step, lo, hi in ((1, 4 * (9 + 0.5 * 999) * 0.99, 4 * (9 + 0.5 * 999) * 1.01), (100000, 0.0, 1e-30)):
        inp = oc.make_inputs(_case(step, "opt"))
        h = oc.HYPER["opt"]
        r = orc.adamw_ema_elementwise(inp["p"], inp["g"], inp["m"], inp["v"], inp["ema"], step, h["lr"], h["betas"],
                                      h["eps"], h["weight_decay"], 1.0, 1.0, h["ema_decay"])
        A_p, A_e = oc.absolute_terms(r, h["betas"], step, h["ema_decay"])
        nz = r["U"] != 0
        ratio = A_p[nz] / (oc.ULP * np.abs(r["U"][nz]))
        assert np.all(ratio >= lo) and np.all(ratio <= hi), (step, ratio.min(), ratio.max())
        assert np.all(A_p[~nz] == 0)
        _close(A_e, (1.0 - F32(h["ema_decay"])) * A_p, "A_e")


def test_restatement_reproduces_the_recorded_figures_and_stays_inside_the_bound():
    """Regenerating golden/optim_achieved.json changes nothing; every case has a record; the recorded maxima times
    the GPU tests' factor stay under K_MAX; no element sits where an ulp of v' is no relative quantity."""
    table = json.load(open(moa.OUT))
    fresh = moa.measure()
    assert json.loads(json.dumps(fresh)) == table
    assert set(table["cases"]) == {c["name"] for c in moa.all_cases()}
    assert table["c_pow"] == oc.C_POW
    for k in moa.OUTPUTS:
        worst = max(rec.get(k, 0.0) for rec in table["cases"].values())
        assert worst == table["max"][k] and 0.0 < worst and oc.K_FACTOR * worst <= oc.K_MAX, (k, worst)
    # the bound with K = the recorded maximum (the GPU tests' K without the factor), case by case, measured afresh
    # (measure() has asserted, element by element, exact agreement wherever a scale is 0)
    for name, rec in fresh["cases"].items():
        assert rec["tiny_sv_share"] == 0.0
        for k in moa.OUTPUTS:
            assert k not in rec or (math.isfinite(rec[k]) and rec[k] <= table["max"][k]), (name, k, rec[k])


def test_without_the_absolute_term_the_first_steps_leave_the_bound():
    """The form of the bound: at steps 2 and 3 the float32 bias corrections alone cost tens of ulps of S_p, which
    A_p absorbs; with it the same cases are back at a few ulps."""
    table = json.load(open(moa.OUT))
    for step in (2, 3):
        case = next(c for c in oc.ADAMW_CASES if c["n"] == oc.N_ROUNDS and c["step"] == step and c["ema"]
                    and c["align"] == "aligned")
        inp = oc.make_inputs(case)
        ref = moa.reference(inp, case, None)
        got = moa.step_f32(inp, case, None)
        raw = np.abs(got["p"].astype(np.float64) - ref["p"]) / (oc.ULP * ref["S_p"])
        assert raw.max() > oc.K_FACTOR * table["max"]["p"], (step, raw.max())
        assert table["cases"][case["name"]]["p"] <= table["max"]["p"]
