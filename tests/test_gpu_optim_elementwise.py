"""The launches of csrc/optim.hip element by element against float64: the clip-norm partials (sumsq, sumsq2), the
clip + AdamW + EMA step (adamw_ema, adamw_ema2) and the bf16 copies the stepping launch writes.

Every buffer is a view into a larger allocation with oc.SENTINEL_FLOATS words of a NaN bit pattern before and after it
(`Arena`); after every launch all words outside the views must be bit-identical, and the inputs a launch only reads
(g, the clip partials) too.  Every output element is compared, none is skipped.

The step is held to  |got - ref| <= K 2^-24 S + A  per element and output (golden/optim_cases.normalised_errors: S
the output's scale from oracle.adamw_ema_elementwise, A what the fp32 bias corrections cost, exact equality where S is
0), with K = optim_cases.K_FACTOR x the maximum that a float32 restatement of the kernel's order of operations
reaches on the CPU over the same cases (golden/optim_achieved.json, written by golden/make_optim_achieved.py and
re-checked by test_optim_elementwise_cpu.py).  The tests print the largest figure they saw per output.
"""
import json

import numpy as np
import pytest
import torch

from golden import make_optim_achieved as moa
from golden import optim_cases as oc

import test_gpu_parity as T

pytestmark = pytest.mark.gpu

_SENT = np.int32(oc.SENTINEL_BITS)
_SENT16 = np.int16(oc.SENTINEL_BITS16)


def _K():
    table = json.load(open(moa.OUT))
    K = {k: oc.K_FACTOR * table["max"][k] for k in moa.OUTPUTS}
    assert all(0.0 < x <= oc.K_MAX for x in K.values()), K
    return K


class Arena:
    """One allocation filled with the sentinel pattern; `specs` = [(name, floats, shifted)] become views with
    SENTINEL_FLOATS words between them, each starting on a 16-byte boundary or (shifted) one float past one."""

    def __init__(self, dev, specs):
        self.off, cur = {}, 0
        for name, n, shifted in specs:
            cur += oc.SENTINEL_FLOATS
            self.off[name] = (cur + (1 if shifted else 0), n)
            cur = (cur + (1 if shifted else 0) + n + 3) // 4 * 4
        cur += oc.SENTINEL_FLOATS
        self.bits = torch.full((cur,), int(_SENT), dtype=torch.int32, device=dev)
        self.f = self.bits.view(torch.float32)
        assert self.f.data_ptr() % 16 == 0
        self.outside = np.ones(cur, dtype=bool)
        for name, n, shifted in specs:
            o = self.off[name][0]
            self.outside[o:o + n] = False
            assert n == 0 or self.view(name).data_ptr() % 16 == (4 if shifted else 0)

    def view(self, name):
        o, n = self.off[name]
        return self.f[o:o + n]

    def put(self, name, arr):
        self.view(name).copy_(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)))

    def get(self, name):
        return self.view(name).cpu().numpy()

    def get_bits(self, name):
        o, n = self.off[name]
        return self.bits[o:o + n].cpu().numpy()

    def check_sentinels(self):
        torch.cuda.synchronize()
        bits = self.bits.cpu().numpy()
        bad = np.nonzero(bits[self.outside] != _SENT)[0]
        assert bad.size == 0, f"{bad.size} words outside the buffers changed, first at {np.nonzero(self.outside)[0][bad[0]]}"


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------ clip-norm partials
def _sumsq_bound(n):
    # the chain of one thread (n / 65536 terms, one fused multiply-add each) plus the trees of the wave, the block and
    # the float64 sum of the parts' roundings; every term is non-negative, so the relative errors add at worst
    return (-(-n // 65536) + 16) * oc.ULP


def _check_parts(parts, g, ones, what):
    assert parts.shape == (256,) and np.all(np.isfinite(parts)), (what, "a partial was not written")
    s = float(parts.astype(np.float64).sum())
    if ones:
        assert s == float(g.size), (what, s, g.size)
        return 0.0
    ref = float((g.astype(np.float64) ** 2).sum())
    rel = abs(s - ref) / ref if ref > 0 else abs(s)
    assert rel <= _sumsq_bound(g.size), (what, rel, _sumsq_bound(g.size))
    return rel / oc.ULP


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("n", oc.SUMSQ_SIZES)
def test_sumsq_partials(n, shifted):
    """sumsq and sumsq2: all 256 partials written over a NaN pre-fill; with g = 1 their sum is n exactly (an element
    missed or counted twice shows); with random g it is within (ceil(n / 65536) + 16) 2^-24 of the float64 sum; the
    step word advances by exactly one per launch.  n = 0 aligned passes a NULL g."""
    from stnf import _native as N
    d = T.dev()
    n1 = oc.N_KNOT_GROUP
    a = Arena(d, [("g", n, shifted), ("parts", 256, False), ("g1", n1, not shifted), ("parts1", 256, False)])
    step = torch.tensor([41], dtype=torch.int32, device=d)
    rs = np.random.RandomState(n + 7 * shifted)
    g1 = rs.standard_normal(n1).astype(np.float32)
    a.put("g1", g1)
    null_g = n == 0 and not shifted
    launches, worst = 0, 0.0
    for ones in (True, False):
        g = np.ones(n, np.float32) if ones else rs.standard_normal(n).astype(np.float32)
        a.put("g", g)
        g_bits, g1_bits = a.get_bits("g"), a.get_bits("g1")
        # one group
        a.view("parts").fill_(float("nan"))
        if null_g:
            N._check(N.lib().stdadk_sumsq_f32(None, 0, _ptr(a.view("parts")), _ptr(step), N._stream()), "sumsq")
        else:
            N.sumsq(a.view("g"), a.view("parts"), step)
        launches += 1
        assert int(step.item()) == 41 + launches
        worst = max(worst, _check_parts(a.get("parts"), g, ones, ("sumsq", n, ones)))
        # two groups: the knot-sized one second, then an empty second group with a NULL pointer
        for second in ("knots", "empty"):
            a.view("parts").fill_(float("nan"))
            a.view("parts1").fill_(float("nan"))
            g0p, g1p, m1 = (None if null_g else _ptr(a.view("g"))), _ptr(a.view("g1")), n1
            if second == "empty":
                g1p, m1 = None, 0
            N._check(N.lib().stdadk_sumsq2_f32(g0p, n, _ptr(a.view("parts")), g1p, m1, _ptr(a.view("parts1")),
                                               _ptr(step), N._stream()), "sumsq2")
            launches += 1
            assert int(step.item()) == 41 + launches, "sumsq2 advances the step once"
            worst = max(worst, _check_parts(a.get("parts"), g, ones, ("sumsq2 group 0", n, ones, second)))
            worst = max(worst, _check_parts(a.get("parts1"), g1[:m1], False, ("sumsq2 group 1", n, second)))
        a.check_sentinels()
        assert np.array_equal(a.get_bits("g"), g_bits) and np.array_equal(a.get_bits("g1"), g1_bits)
    print(f"sumsq n={n} {'shifted' if shifted else 'aligned'}: worst {worst:.2f} of {_sumsq_bound(n) / oc.ULP:.0f} ulps")


# ------------------------------------------------------------------ the step
_FIVE = ("p", "g", "m", "v", "ema")


def _load(a, inp, suffix=""):
    for k in _FIVE:
        if inp[k] is not None:
            a.put(k + suffix, inp[k])
    if inp["parts"] is not None:
        a.put("parts" + suffix, inp["parts"])


def _specs(case, suffix=""):
    shifted = oc.ALIGNMENTS[case["align"]]
    specs = [(k + suffix, case["n"], k in shifted) for k in _FIVE if k != "ema" or case["ema"]]
    if case["clip"] is not None:
        specs.append(("parts" + suffix, 256 if case["clip"] == "sumsq" else case["clip"][1], False))
    return specs


def _outputs(a, case, suffix=""):
    return {k: (a.get(k + suffix) if k != "ema" or case["ema"] else None) for k in ("p", "m", "v", "ema")}


def _launch(N, a, case, dev, suffix=""):
    """The single-group launch of `case` on the arena's views (the environment is the caller's)."""
    h = oc.case_hyper(case)
    lr, step, lr_dev, step_dev = h["lr"], case["step"], None, None
    if case.get("dev_args"):
        lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev)
        step_dev = torch.tensor([step], dtype=torch.int32, device=dev)
        lr, step = 123.0, 77                  # must be ignored
    clip = case["clip"] is not None
    N.adamw_ema(a.view("p" + suffix), a.view("g" + suffix), a.view("m" + suffix), a.view("v" + suffix),
                a.view("ema" + suffix) if case["ema"] else None, lr, h["betas"], h["eps"], h["weight_decay"], step,
                max_norm=h["max_norm"] if clip else 0.0, sumsq_parts=a.view("parts" + suffix) if clip else None,
                grad_mul=case["grad_mul"], ema_decay=h["ema_decay"], lr_dev=lr_dev, step_dev=step_dev)


def _compare(case, inp, parts, got, K, seen):
    """[what is wrong] of one case's outputs against the float64 reference under the bound."""
    h = oc.case_hyper(case)
    ref = moa.reference(inp, case, parts)
    bad = []
    for k, (e, exact) in oc.normalised_errors(got, ref, h["betas"], case["step"], h["ema_decay"]).items():
        seen[k] = max(seen.get(k, 0.0), e)
        if not exact:
            bad.append(f"{case['name']} {k}: differs from the reference where its scale is 0")
        if not e <= K[k]:
            bad.append(f"{case['name']} {k}: {e:.2f} ulps of S, K = {K[k]:.2f}")
    return bad


def _run_cases(case_list, monkeypatch):
    from stnf import _native as N
    d, K, seen, bad = T.dev(), _K(), {}, []
    assert case_list
    for case in case_list:
        if case["blocks"] is None:
            monkeypatch.delenv("STDADK_ADAMW_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("STDADK_ADAMW_BLOCKS", str(case["blocks"]))
        inp = oc.make_inputs(case)
        a = Arena(d, _specs(case))
        _load(a, inp)
        parts = inp["parts"]
        if case["clip"] == "sumsq":
            N.sumsq(a.view("g"), a.view("parts"))
            parts = a.get("parts")
        g_bits = a.get_bits("g")
        parts_bits = a.get_bits("parts") if parts is not None else None
        _launch(N, a, case, d)
        a.check_sentinels()
        assert np.array_equal(a.get_bits("g"), g_bits), (case["name"], "the gradient was written")
        assert parts is None or np.array_equal(a.get_bits("parts"), parts_bits), (case["name"], "partials written")
        bad += _compare(case, inp, parts, _outputs(a, case), K, seen)
    print("adamw_ema", len(case_list), "cases, largest normalised error (ulps of S):",
          {k: round(v, 2) for k, v in seen.items()}, "K:", {k: round(v, 2) for k, v in K.items()})
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("n", oc.SMALL_SIZES + (oc.N_ROUNDS, oc.N_STRIDE))
def test_adamw_ema_sizes_alignments_steps(n, monkeypatch):
    """Every alignment, with and without a shadow, every step of oc.STEPS, both hyper-parameter sets: the float4 body,
    its prefetch, the scalar tail, the all-scalar fallback, the reload of later rounds (n = 2055 on one block) and the
    second grid-stride round (n = 1572887)."""
    _run_cases([c for c in oc.ADAMW_CASES if c["name"].startswith(f"n{n}_")], monkeypatch)


def test_adamw_ema_clipping(monkeypatch):
    """Hand-filled partials with the norm at 0, 0.999, 1.001 and 1000 x max_norm in 1, 255, 256, 512 and 2567 parts,
    and two cases whose partials come from the sumsq launch; the reference coefficient is float64 from the same
    partials; grad_mul = 0.25."""
    _run_cases([c for c in oc.ADAMW_CASES if c["name"].startswith("clip_")], monkeypatch)


def test_adamw_ema_device_words_take_precedence(monkeypatch):
    """lr_dev and step_dev win over the scalar lr and step (which hold 123 and 77 here)."""
    cs = [c for c in oc.ADAMW_CASES if c["dev_args"]]
    assert len(cs) == 2
    _run_cases(cs, monkeypatch)


def test_nonfinite_guard_records_the_first_bad_step():
    """A watched +inf or NaN writes the step into a zero word; a later bad step does not overwrite it; a finite value
    leaves it 0.  The step comes from the scalar or from the device word."""
    from stnf import _native as N
    d = T.dev()
    case = next(c for c in oc.ADAMW_CASES if c["name"] == "n1027_aligned_ema_t3")
    h = oc.case_hyper(case)
    a = Arena(d, _specs(case))

    def run(watch_value, step, word, step_dev=None):
        _load(a, oc.make_inputs(case))
        watch = torch.tensor([watch_value], dtype=torch.float32, device=d)
        N.adamw_ema(a.view("p"), a.view("g"), a.view("m"), a.view("v"), a.view("ema"), h["lr"], h["betas"], h["eps"],
                    h["weight_decay"], step, ema_decay=h["ema_decay"], step_dev=step_dev, loss_watch=watch,
                    nonfinite_step=word)
        return int(word.item())

    word = torch.zeros(1, dtype=torch.int32, device=d)
    assert run(3.0e38, 5, word) == 0
    assert run(-1.5, 6, word) == 0
    assert run(float("inf"), 7, word) == 7
    assert run(float("nan"), 9, word) == 7
    assert run(1.0, 10, word) == 7
    word2 = torch.zeros(1, dtype=torch.int32, device=d)
    assert run(float("nan"), 77, word2, torch.tensor([4], dtype=torch.int32, device=d)) == 4
    assert run(float("-inf"), 77, word2, torch.tensor([5], dtype=torch.int32, device=d)) == 4
    a.check_sentinels()


# ------------------------------------------------------------------ two groups in one launch
@pytest.mark.parametrize("c2", oc.ADAMW2_CASES, ids=[c["name"] for c in oc.ADAMW2_CASES])
def test_adamw_ema2_equals_two_single_launches(c2, monkeypatch):
    """One launch over two groups (own lr, max_norm and partials each) == two single-group launches on copies of the
    same buffers, bit for bit (sentinels included); both groups also against the float64 reference."""
    from stnf import _native as N
    monkeypatch.delenv("STDADK_ADAMW_BLOCKS", raising=False)
    d, K, seen, bad = T.dev(), _K(), {}, []
    gcs = [oc.adamw2_group_case(c2, i) for i in range(2)]
    inps = [oc.make_inputs(c) for c in gcs]
    a = Arena(d, _specs(gcs[0], "0") + _specs(gcs[1], "1"))
    for i in range(2):
        _load(a, inps[i], str(i))
    b = Arena(d, _specs(gcs[0], "0") + _specs(gcs[1], "1"))
    b.bits.copy_(a.bits)
    hs = [oc.case_hyper(c) for c in gcs]
    groups = [N.make_adam_group(*(a.view(k + str(i)) for k in _FIVE), hs[i]["lr"], max_norm=hs[i]["max_norm"],
                                sumsq_parts=a.view("parts" + str(i))) for i in range(2)]
    h = hs[0]
    N.adamw_ema2(groups[0], groups[1], h["betas"], h["eps"], h["weight_decay"], c2["step"], grad_mul=c2["grad_mul"],
                 ema_decay=h["ema_decay"])
    for i in range(2):
        _launch(N, b, gcs[i], d, str(i))
    a.check_sentinels()
    assert torch.equal(a.bits, b.bits), "the two-group launch differs from two single-group launches"
    for i in range(2):
        bad += _compare(gcs[i], inps[i], inps[i]["parts"], _outputs(a, gcs[i], str(i)), K, seen)
    print("adamw_ema2", c2["name"], "largest normalised error (ulps of S):", {k: round(v, 2) for k, v in seen.items()})
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ bf16 copies written by the stepping launch
@pytest.mark.parametrize("blocks", oc.BF16_BLOCKS, ids=["one_block", "default_grid"])
def test_bf16_copies_follow_the_step(blocks, monkeypatch):
    """The plain and the transposed copy of every region == torch's cast of the stepped parameters, bit for bit; the
    stepped values are those of a launch without copies; what lies outside the regions in copy buffers one row larger
    (and 64 halves before and after) is untouched.  The second region ends where the float4 body ends (n % 4 == 3)."""
    from stnf import _native as N
    if blocks is None:
        monkeypatch.delenv("STDADK_ADAMW_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("STDADK_ADAMW_BLOCKS", str(blocks))
    d = T.dev()
    n = oc.BF16_N
    assert n % 4 == 3 and oc.BF16_REGIONS[1][0] + 64 * 36 == n - 3
    case = dict(name="bf16_copies", n=n, align="aligned", ema=True, step=3, hyper="opt", grad_mul=1.0, clip=None,
                blocks=blocks, dev_args=False)
    inp = oc.make_inputs(case)
    a, plain = Arena(d, _specs(case)), Arena(d, _specs(case))
    _load(a, inp)
    _load(plain, inp)
    pad, bufs, regions = oc.SENTINEL_FLOATS, [], []
    for off, rows, cols in oc.BF16_REGIONS:
        wb = torch.full((pad + (rows + 1) * cols + pad,), int(_SENT16), dtype=torch.int16, device=d)
        wt = torch.full((pad + (cols + 1) * rows + pad,), int(_SENT16), dtype=torch.int16, device=d)
        bufs.append((wb, wt))
        regions.append((off, rows, cols, wb.view(torch.bfloat16)[pad:pad + rows * cols],
                        wt.view(torch.bfloat16)[pad:pad + rows * cols]))
    h = oc.case_hyper(case)
    sh = N.make_bf16_shadow(regions)
    N.adamw_ema(a.view("p"), a.view("g"), a.view("m"), a.view("v"), a.view("ema"), h["lr"], h["betas"], h["eps"],
                h["weight_decay"], case["step"], ema_decay=h["ema_decay"], shadow=sh)
    _launch(N, plain, case, d)
    a.check_sentinels()
    assert torch.equal(a.bits, plain.bits), "the copies' pass changed what the step computes"
    p = a.view("p")
    for (off, rows, cols), (wb, wt) in zip(oc.BF16_REGIONS, bufs):
        want = p[off:off + rows * cols].view(rows, cols).bfloat16()
        cnt = rows * cols
        assert torch.equal(wb[pad:pad + cnt], want.view(torch.int16).reshape(-1)), (off, "plain copy")
        assert torch.equal(wt[pad:pad + cnt], want.t().contiguous().view(torch.int16).reshape(-1)), (off, "transposed")
        for buf in (wb, wt):
            rest = torch.cat([buf[:pad], buf[pad + cnt:]])
            assert bool((rest == int(_SENT16)).all()), (off, "written outside the region")
