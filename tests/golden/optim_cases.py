"""Cases, inputs and the error bound of the per-element optimiser tests (tests/test_gpu_optim_elementwise.py, the
CPU half in tests/test_optim_elementwise_cpu.py, the recorded figures of make_optim_achieved.py).

Numpy only and deterministic (numpy.random.RandomState), like cases.py: the GPU box rebuilds every input.

A case of ADAMW_CASES is a dict:
  name       unique
  n          elements
  align      which of the five buffers start one float past a 16-byte boundary (ALIGNMENTS)
  ema        an EMA shadow is given (False: NULL)
  step       the step counter t (1: m = v = 0)
  hyper      key of HYPER
  grad_mul   the factor on the gradient next to the clip coefficient
  clip       None (max_norm 0, no partials), "sumsq" (partials from the sumsq launch itself) or
             (norm / max_norm, n_parts): hand-filled partials whose root is that multiple of max_norm
  blocks     None (the launch's own grid) or the value of STDADK_ADAMW_BLOCKS
  dev_args   lr and step come from device words; the scalar arguments then hold values that must be ignored
"""
import math

import numpy as np

from golden import cases

SENTINEL_FLOATS = 64
SENTINEL_BITS = 0x7FC5A5A5            # a quiet NaN with a payload no arithmetic produces
SENTINEL_BITS16 = 0x7FC5              # the same for the bf16 copies

STEPS = (1, 2, 3, 10, 1000, 100000)
ALIGNMENTS = {"aligned": (), "all": ("p", "g", "m", "v", "ema"), "g": ("g",), "ema": ("ema",)}

_O = cases.OPT
HYPER = {
    "opt": dict(lr=_O["lr"], weight_decay=_O["weight_decay"], betas=_O["betas"], eps=_O["eps"],
                ema_decay=_O["ema_decay"], max_norm=_O["grad_clip"]),
    # strong decoupled decay and gradients around eps: decay folded into the gradient, or eps under the square root,
    # are each wrong by far more than the bound here
    "wd": dict(lr=1e-2, weight_decay=0.1, betas=_O["betas"], eps=1e-8, ema_decay=_O["ema_decay"],
               max_norm=_O["grad_clip"]),
}

C_POW = 4.0             # ulps allowed to powf in the bias corrections (A_p below)
K_FACTOR = 4.0          # GPU bound = K_FACTOR x the recorded CPU maximum: FMA contraction, the hardware's division and
                        # square-root sequences, powf -- none of which numpy reproduces
K_MAX = 64.0
ULP = 2.0 ** -24

# sizes: 1, 3 (tail only), 4 (one group), 5 (group + tail), 1027 (two blocks, 3-element tail); 2055 under
# STDADK_ADAMW_BLOCKS=1: 513 groups on 256 threads = three rounds for thread 0 (the reload of rounds after the first)
# plus a tail; 1572887 = 4 * 1536 * 256 + 23: the smallest size whose second grid-stride round is not empty (5 groups),
# with a 3-element tail
SMALL_SIZES = (1, 3, 4, 5, 1027)
N_ROUNDS = 2055
N_STRIDE = 1572887
SUMSQ_SIZES = (0, 1, 3, 4, 5, 1023, 1025, 262147, 1572887)
N_KNOT_GROUP = 681      # 227 learnable knots x (x, y, log bandwidth)
N_MLP_GROUP = 12932
CLIP_RATIOS = (0.0, 0.999, 1.001, 1000.0)
CLIP_PARTS = (1, 255, 256, 512, 2567)


def _case(name, n, align="aligned", ema=True, step=1, hyper="opt", grad_mul=1.0, clip=None, blocks=None,
          dev_args=False):
    return dict(name=name, n=n, align=align, ema=ema, step=step, hyper=hyper, grad_mul=grad_mul, clip=clip,
                blocks=blocks, dev_args=dev_args)


def _sweep(n, blocks=None):
    """every alignment x shadow given / NULL x every step, hyper set and grad_mul alternating"""
    out, k = [], 0
    for align in ALIGNMENTS:
        for ema in (True, False):
            if align == "ema" and not ema:
                continue
            for step in STEPS:
                out.append(_case(f"n{n}_{align}_{'ema' if ema else 'noema'}_t{step}", n, align, ema, step,
                                 "wd" if k % 2 else "opt", 0.25 if k % 3 == 0 else 1.0, None, blocks))
                k += 1
    return out


def _adamw_cases():
    out = []
    for n in SMALL_SIZES:
        out += _sweep(n)
    out += _sweep(N_ROUNDS, blocks=1)
    # the default grid's second round: every alignment, both hyper sets, shadow given and NULL (five cases: the float64
    # reference of 1.6 M elements costs a second each)
    big = [("aligned", True, 1, "opt"), ("aligned", False, 2, "wd"), ("all", True, 3, "wd"), ("g", True, 1000, "opt"),
           ("ema", True, 100000, "wd")]
    for align, ema, step, hyper in big:
        out.append(_case(f"n{N_STRIDE}_{align}_{'ema' if ema else 'noema'}_t{step}", N_STRIDE, align, ema, step,
                         hyper, 0.25 if step == 3 else 1.0))
    # clipping: hand-filled partials around the edge, every partial count; grad_mul 0.25 throughout
    k = 0
    for ratio in CLIP_RATIOS:
        for n_parts in CLIP_PARTS:
            out.append(_case(f"clip_r{ratio:g}_parts{n_parts}", 1027, "aligned", True, STEPS[1 + k % 5],
                             "wd" if k % 2 else "opt", 0.25, (ratio, n_parts)))
            k += 1
    out.append(_case("clip_through_sumsq", 1027, "aligned", True, 3, "opt", 0.25, "sumsq"))
    out.append(_case("clip_through_sumsq_big", 12932, "all", True, 10, "wd", 0.25, "sumsq"))
    # lr and step from device words
    out.append(_case("dev_args_t1", 1027, "aligned", True, 1, "opt", 1.0, (1.001, 256), None, True))
    out.append(_case("dev_args_t1000", 1027, "all", False, 1000, "wd", 0.25, None, None, True))
    return out


ADAMW_CASES = _adamw_cases()
assert len({c["name"] for c in ADAMW_CASES}) == len(ADAMW_CASES)

# the two-group launch: (group 0 = knots, group 1 = MLP), each a case above in all but name
ADAMW2_CASES = [
    dict(name="knots681_mlp12932", step=3, hyper="wd", grad_mul=0.25,
         groups=[dict(n=N_KNOT_GROUP, lr_mul=cases.BASIS_LR_RATIO, clip=(1.001, 256), max_norm_mul=cases.BASIS_CLIP_RATIO),
                 dict(n=N_MLP_GROUP, lr_mul=1.0, clip=(1000.0, 256), max_norm_mul=1.0)]),
    dict(name="n5_n1572887", step=2, hyper="opt", grad_mul=1.0,
         groups=[dict(n=5, lr_mul=0.5, clip=(0.999, 256), max_norm_mul=0.1),
                 dict(n=N_STRIDE, lr_mul=1.0, clip=(1.001, 512), max_norm_mul=1.0)]),
]

# bf16 copies inside the stepping launch: (offset, rows, cols); n % 4 == 3 and the second region ends at n - 3
BF16_N = 4099
BF16_REGIONS = ((0, 16, 32), (BF16_N - 3 - 64 * 36, 64, 36))
BF16_BLOCKS = (1, None)


def adamw2_group_case(c2, i):
    """Group i of an ADAMW2_CASES entry as a single-group case (aligned, with a shadow, own lr and max_norm)."""
    gr = c2["groups"][i]
    c = _case(f"{c2['name']}_g{i}", gr["n"], "aligned", True, c2["step"], c2["hyper"], c2["grad_mul"], gr["clip"])
    c.update(lr_mul=gr["lr_mul"], max_norm_mul=gr["max_norm_mul"])
    return c


def case_hyper(case):
    """The case's hyper-parameters: HYPER[case['hyper']] with the group's own lr and max_norm (two-group cases)."""
    h = dict(HYPER[case["hyper"]])
    h["lr"] *= case.get("lr_mul", 1.0)
    h["max_norm"] *= case.get("max_norm_mul", 1.0)
    return h


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31 - 1)


def _magnitudes(rs, n, lo=-30, hi=2):
    """Spread evenly over the binades 2^lo .. 2^hi (1.0e-9 .. 7.6 by default) with exact arithmetic only: no libm
    function whose last bit could differ between machines."""
    return np.ldexp(rs.uniform(1.1, 1.9, size=n), rs.randint(lo, hi + 1, size=n))


def _signs(rs, n):
    return np.where(rs.randint(0, 2, size=n) == 1, 1.0, -1.0)


def make_parts(rs, clip, max_norm):
    """`n_parts` positive float32 partials whose sum is (ratio * max_norm)^2 up to rounding (all zero for ratio 0)."""
    ratio, n_parts = clip
    w = rs.uniform(0.5, 1.5, size=n_parts)
    return ((ratio * max_norm) ** 2 * w / w.sum()).astype(np.float32)


def make_inputs(case):
    """float32 p, g, m, v, ema (None without a shadow) and hand-filled `parts` (None unless clip is a pair).
    |g|, |m| and sqrt(v) are spread over 1e-9 .. 7.6; every tenth gradient is exactly 0; with the "wd" set another
    tenth lies in [1e-9, 5.7e-8]; at step 1 m = v = 0.  No value and no product the step forms is subnormal."""
    n, rs = case["n"], np.random.RandomState(_seed(case["name"]))
    i = np.arange(n)
    g = _signs(rs, n) * _magnitudes(rs, n)
    if case["hyper"] == "wd":
        g = np.where(i % 10 == 5, _signs(rs, n) * _magnitudes(rs, n, -30, -25), g)
    g = np.where(i % 10 == 2, 0.0, g)
    p = rs.standard_normal(n)
    m = _signs(rs, n) * _magnitudes(rs, n)
    v = _magnitudes(rs, n) ** 2
    if case["step"] == 1:
        m, v = np.zeros(n), np.zeros(n)
    ema = p + 0.01 * rs.standard_normal(n)
    out = {k: a.astype(np.float32) for k, a in dict(p=p, g=g, m=m, v=v, ema=ema).items()}
    assert np.all((np.abs(out["g"]) >= 1e-12) | (out["g"] == 0.0))
    if not case["ema"]:
        out["ema"] = None
    out["parts"] = None
    if isinstance(case["clip"], tuple):
        out["parts"] = make_parts(rs, case["clip"], case_hyper(case)["max_norm"])
    return out


def clip_coef64(parts, max_norm):
    """The clip coefficient in float64 from float32 partials (max_norm and the 1e-6 rounded to float32 as the kernel
    has them); 1 without clipping."""
    if parts is None or not max_norm > 0:
        return 1.0
    ss = float(np.asarray(parts, dtype=np.float64).sum())
    return min(1.0, float(np.float32(max_norm)) / (math.sqrt(ss) + float(np.float32(1e-6))))


def absolute_terms(ref, betas, step, ema_decay, c_pow=C_POW):
    """(A_p, A_e): what the fp32 bias corrections 1 - powf(beta, t) cost.  powf is off by up to c_pow ulps of
    beta^t, i.e. c_pow 2^-24 beta^t / (1 - beta^t) of the correction: on lr/bc1 in full, on sqrt(bc2) by half."""
    b1, b2, d = (float(np.float32(x)) for x in (betas[0], betas[1], ema_decay))
    A_p = c_pow * ULP * (b1 ** step / ref["bc1"] + 0.5 * b2 ** step / ref["bc2"]) * np.abs(ref["U"])
    return A_p, (1.0 - d) * A_p


def normalised_errors(got, ref, betas, step, ema_decay):
    """{output: (largest (|got - ref| - A) / (2^-24 S) over the elements with S > 0, every element with S == 0 equal
    to the reference)} for p, m, v and (when there is one) ema.  No element is left out."""
    A_p, A_e = absolute_terms(ref, betas, step, ema_decay)
    out = {}
    for k, S, A in (("p", ref["S_p"], A_p), ("m", ref["S_m"], 0.0), ("v", ref["S_v"], 0.0), ("ema", ref["S_e"], A_e)):
        if ref[k] is None:
            continue
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])
        assert err.shape == S.shape
        pos = S > 0
        exact = bool(np.all(err[~pos] == 0.0))
        ulps = np.maximum(err - A, 0.0)[pos] / (ULP * S[pos]) if pos.any() else np.zeros(1)
        worst = float(ulps.max()) if np.all(np.isfinite(ulps)) else float("inf")
        out[k] = (worst, exact)
    return out
