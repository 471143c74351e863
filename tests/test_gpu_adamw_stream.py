"""The float4 stream of the clip + AdamW + EMA launch (csrc/optim.hip: adamw_ema_block) where a change to its loop can
go wrong: the number of groups a thread walks (the first group loaded ahead of the prologue, the reload of later ones,
the last group partly filled, and -- for any form that prefetches -- the index one group past the end), the number of
clip-norm partials against the unrolled loads (and the order of their additions), and the operand copies written from a
group's registers wherever the group lies in its thread's walk.

Comparator, guarded arena (NaN sentinels around every buffer) and float64 oracle are those of
test_gpu_optim_elementwise.py; the bound K is the same.  Cases: golden/adamw_stream_cases.py.
"""
import numpy as np
import pytest
import torch

from golden import adamw_stream_cases as sc
from golden import make_adamw_stream_expected as mk
from golden import optim_cases as oc

import test_gpu_optim_elementwise as E
import test_gpu_parity as T

pytestmark = pytest.mark.gpu


def _run(N, d, case, blocks, monkeypatch):
    """(arena after the launch, inputs) of `case` under STDADK_ADAMW_BLOCKS = blocks (None: the launch's own grid)."""
    if blocks is None:
        monkeypatch.delenv("STDADK_ADAMW_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("STDADK_ADAMW_BLOCKS", str(blocks))
    inp = oc.make_inputs(case)
    a = E.Arena(d, E._specs(case))
    E._load(a, inp)
    g_bits = a.get_bits("g")
    E._launch(N, a, case, d)
    a.check_sentinels()
    assert np.array_equal(a.get_bits("g"), g_bits), (case["name"], "the gradient was written")
    return a, inp


# ------------------------------------------------------------------ groups per thread
@pytest.mark.parametrize("blocks", sc.GROUP_BLOCKS)
def test_groups_per_thread(blocks, monkeypatch):
    """1 .. 5 groups per thread under a forced grid (n = 4 (k stride + r) + t): every output within K of the float64
    oracle, sentinels intact, and the launch's own grid bit-identical to the forced one -- aligned and shifted by
    4 bytes (scalar path), with and without an EMA buffer."""
    from stnf import _native as N
    d, K, seen, bad = T.dev(), E._K(), {}, []
    case_list = sc.group_cases(blocks)
    assert len(case_list) == 4 * 3 * 2 * 4
    for case in case_list:
        forced, inp = _run(N, d, case, blocks, monkeypatch)
        own, _ = _run(N, d, case, None, monkeypatch)
        assert torch.equal(forced.bits, own.bits), (case["name"], "the result depends on the grid")
        bad += E._compare(case, inp, None, E._outputs(forced, case), K, seen)
    print(f"stream, {blocks} block(s):", len(case_list), "cases, largest normalised error (ulps of S):",
          {k: round(v, 2) for k, v in seen.items()}, "K:", {k: round(v, 2) for k, v in K.items()})
    assert not bad, "\n".join(bad[:20])


# ------------------------------------------------------------------ partial counts
@pytest.mark.parametrize("n_parts", sc.PART_COUNTS)
def test_partials_exact_sum(n_parts, monkeypatch):
    """Integer partials: their sum is exact in any order, so the coefficient is known and the outputs compare against
    the oracle with it.  NaNs lie behind the partials: one that is loaded and added makes every output NaN."""
    monkeypatch.delenv("STDADK_ADAMW_BLOCKS", raising=False)
    case = sc.parts_case("int", n_parts)
    parts = sc.make_parts(case)
    assert float(parts.astype(np.float64).sum()) < 2.0 ** 24 and float(parts.sum()) > oc.HYPER["opt"]["max_norm"] ** 2
    got, _, inp = mk.run_parts_case(case, parts)
    seen = {}
    bad = E._compare(case, inp, parts, got, E._K(), seen)
    print("integer partials", n_parts, {k: round(v, 2) for k, v in seen.items()})
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n_parts", sc.PART_COUNTS)
def test_partials_keep_the_order_of_the_additions(n_parts, monkeypatch):
    """Partials spread over 2^-20 .. 2^20: the outputs equal, bit for bit, those recorded from the library that summed
    them one dependent load at a time (golden/adamw_stream_expected.npz)."""
    monkeypatch.delenv("STDADK_ADAMW_BLOCKS", raising=False)
    case = sc.parts_case("spread", n_parts)
    got, _, _ = mk.run_parts_case(case, sc.make_parts(case))
    rec = np.load(mk.OUT)
    for k in mk.OUTPUTS:
        want = rec[f"{k}_{n_parts}"]
        assert want.dtype == np.int32 and want.shape == (sc.PARTS_N,)
        diff = np.nonzero(got[k].view(np.int32) != want)[0]
        assert diff.size == 0, (k, n_parts, f"{diff.size} of {want.size} elements differ from the recorded bits")


# ------------------------------------------------------------------ copies by position
def _bf16_buffers(d, regions):
    """[(off, rows, cols, plain, transposed)] over sentinel-filled int16 buffers, and the buffers."""
    pad, bufs, table = oc.SENTINEL_FLOATS, [], []
    for off, rows, cols in regions:
        wb = torch.full((pad + rows * cols + pad,), int(E._SENT16), dtype=torch.int16, device=d)
        wt = torch.full((pad + rows * cols + pad,), int(E._SENT16), dtype=torch.int16, device=d)
        bufs += [wb, wt]
        table.append((off, rows, cols, wb.view(torch.bfloat16)[pad:pad + rows * cols],
                      wt.view(torch.bfloat16)[pad:pad + rows * cols]))
    return table, bufs


def _copy_case():
    return oc._case("stream_copies", sc.COPY_N, "aligned", True, 3, "opt", 1.0, None)


@pytest.mark.parametrize("blocks", sc.COPY_BLOCKS)
@pytest.mark.parametrize("position", list(sc.COPY_POSITIONS))
def test_bf16_copies_by_position(position, blocks, monkeypatch):
    """The copies the stepping launch writes == what the refresh launch writes from the stepped parameters, bit for
    bit (padding included), the regions being a thread's first, a middle or its last group; the step itself is that
    of a launch without copies."""
    from stnf import _native as N
    monkeypatch.setenv("STDADK_ADAMW_BLOCKS", str(blocks))
    d, case = T.dev(), _copy_case()
    inp, h = oc.make_inputs(case), oc.case_hyper(case)
    a, plain = E.Arena(d, E._specs(case)), E.Arena(d, E._specs(case))
    E._load(a, inp)
    E._load(plain, inp)
    regions = sc.copy_regions(position)
    table, bufs = _bf16_buffers(d, regions)
    N.adamw_ema(a.view("p"), a.view("g"), a.view("m"), a.view("v"), a.view("ema"), h["lr"], h["betas"], h["eps"],
                h["weight_decay"], case["step"], ema_decay=h["ema_decay"], shadow=N.make_bf16_shadow(table))
    E._launch(N, plain, case, d)
    a.check_sentinels()
    assert torch.equal(a.bits, plain.bits), "the copies changed what the step computes"
    table2, bufs2 = _bf16_buffers(d, regions)
    N.bf16_shadow_refresh(a.view("p"), N.make_bf16_shadow(table2))
    torch.cuda.synchronize()
    for got, want in zip(bufs, bufs2):
        assert torch.equal(got, want), (position, blocks)
    assert not bool((bufs2[0][oc.SENTINEL_FLOATS:-oc.SENTINEL_FLOATS] == int(E._SENT16)).all())   # the refresh wrote


def test_bf16_copies_of_the_two_group_launch(monkeypatch):
    """adamw_ema2_kernel with the regions in group 0, next to a knot-sized group 1: copies == refresh, and both groups
    == two single-group launches."""
    from stnf import _native as N
    monkeypatch.delenv("STDADK_ADAMW_BLOCKS", raising=False)
    d = T.dev()
    c0 = dict(_copy_case(), name="stream_copies_g0")
    c1 = oc._case("stream_copies_g1", oc.N_KNOT_GROUP, "aligned", True, 3, "opt", 1.0, None)
    hs = [oc.case_hyper(c0), dict(oc.case_hyper(c1), lr=oc.case_hyper(c1)["lr"] * 0.05)]
    inps = [oc.make_inputs(c0), oc.make_inputs(c1)]
    specs = E._specs(c0, "0") + E._specs(c1, "1")
    a, b = E.Arena(d, specs), E.Arena(d, specs)
    for i in range(2):
        E._load(a, inps[i], str(i))
    b.bits.copy_(a.bits)
    regions = sc.copy_regions("end")
    table, bufs = _bf16_buffers(d, regions)
    g0 = N.make_adam_group(*(a.view(k + "0") for k in E._FIVE), hs[0]["lr"], shadow=N.make_bf16_shadow(table))
    g1 = N.make_adam_group(*(a.view(k + "1") for k in E._FIVE), hs[1]["lr"])
    h = hs[0]
    N.adamw_ema2(g0, g1, h["betas"], h["eps"], h["weight_decay"], 3, grad_mul=1.0, ema_decay=h["ema_decay"])
    for i, c in enumerate((c0, c1)):
        N.adamw_ema(*(b.view(k + str(i)) for k in E._FIVE), hs[i]["lr"], h["betas"], h["eps"], h["weight_decay"], 3,
                    ema_decay=h["ema_decay"])
    a.check_sentinels()
    assert torch.equal(a.bits, b.bits), "the two-group launch differs from two single-group launches"
    table2, bufs2 = _bf16_buffers(d, regions)
    N.bf16_shadow_refresh(a.view("p0"), N.make_bf16_shadow(table2))
    torch.cuda.synchronize()
    for got, want in zip(bufs, bufs2):
        assert torch.equal(got, want)


@pytest.mark.parametrize("blocks", sc.COPY_BLOCKS)
def test_packed_copies_of_a_step_under_forced_grids(blocks, monkeypatch):
    """The fragment-order fp32 copies have no launch of their own: a one-call training step keeps them (hidden 128 x
    48 and 48 x 64 behind W0 in the flat buffer: middle and last groups of a thread under these grids).  After the step
    they equal what stdadk_f32_pack_refresh writes from the stepped parameters, bit for bit."""
    from stnf import _native as N
    import test_gpu_packed_weights as PW
    monkeypatch.setenv("STDADK_ADAMW_BLOCKS", str(blocks))
    B = PW.B_RAGGED
    eng = PW._engine([128, 48, 64], B, True)
    coords, t, y = PW._data(B, 21)
    eng.step(None, coords, t, y)
    torch.cuda.synchronize()
    fresh = [(off, h, hp, torch.full_like(pf, float("nan")), torch.full_like(pb, float("nan")))
             for off, h, hp, pf, pb in eng._pack_regions]
    N.f32_pack_refresh(eng.flat, N.make_bf16_shadow(fresh))
    torch.cuda.synchronize()
    assert len(fresh) == 2
    for (_, h, hp, pf, pb), (_, _, _, pf2, pb2) in zip(eng._pack_regions, fresh):
        assert torch.equal(pf.view(torch.int32), pf2.view(torch.int32)), (h, hp, "forward copy")
        assert torch.equal(pb.view(torch.int32), pb2.view(torch.int32)), (h, hp, "backward copy")
