"""Fragment-order fp32 copies of the hidden weights (STDADK_FLAG_PACK_F32; PF / PB of include/stdadk.h): the fused tail
kernels stream a wave's weight fragments from them as contiguous KiB instead of 16 row pieces.  The copies re-address
operands and re-order no sum, so every comparison here is exact (torch.equal / np.array_equal) -- but for the running
loss sum, which the workgroups of a launch add to with float atomics in the order they arrive: two runs of ONE build
differ in its last bits, so it is held to the bound that a re-ordered float32 sum of its non-negative terms allows
(loss_reorder_bound below) while everything computed from the rows themselves must be equal:
  * the layout stdadk_f32_pack_refresh writes, against the two formulas of the header in numpy;
  * one-call steps with and without the flag from the same state: loss, gradients, parameters, moments, EMA;
  * the copies the optimiser launch keeps, against the packing of the weights it has just stepped;
  * TrainStep's lifecycle (EMA swaps, load_state_dict, hipGraph replay) with pack_weights on and off;
  * the two error paths of the flag.

Batch sizes of the step tests, from the launch plan (mlp.hip / tail.hip: l1_tail_supported, tail_rows): up to 4 096
rows on the window path the step runs l1_tail_kernel (16-row tiles; 37 = a ragged last tile, 4 096 = every CU);
beyond, tail_fwd_bwd_kernel with 32-row tiles from ceil(B / 32) >= 256, i.e. B = 8 161, and with 64-row tiles from
ceil(B / 64) >= 256, i.e. B = 16 321."""
import functools

import numpy as np
import pytest
import torch

from golden import cases

import test_gpu_parity as T

pytestmark = pytest.mark.gpu

B_RAGGED, B_L1_TAIL, B_ROWS32, B_ROWS64 = 37, 4096, 8161, 16321
KERNEL_OF = {B_RAGGED: "l1_tail_kernel", B_L1_TAIL: "l1_tail_kernel", B_ROWS32: "tail_fwd_bwd_kernel",
             B_ROWS64: "tail_fwd_bwd_kernel"}
HIDDEN = ([256, 256, 128], [128, 48, 64])


def loss_reorder_bound(B, rows_per_wg, steps=3):
    """Relative bound between two float32 sums of the same n non-negative terms taken in different orders: each is
    within (n - 1) u of the exact sum, u = 2^-24; n = one atomic add per workgroup and step."""
    n = steps * -(-B // rows_per_wg)
    return 2 * (n - 1) * 2.0 ** -24


ROWS_PER_WG = {B_RAGGED: 16, B_L1_TAIL: 16, B_ROWS32: 32, B_ROWS64: 64}


# ------------------------------------------------------------------------------------------------ numpy packing
def pack_np(M):
    """M[n][k], the [N][K] operand -> its packed copy: out[c][nt][j][lane][e] = M[16 nt + c16][32 c + 16 j + 4 q + e],
    lane = 16 q + c16, zero beyond K."""
    Nn, K = M.shape
    NT, NCH = Nn // 16, (K + 31) // 32
    Mp = np.zeros((Nn, 32 * NCH), M.dtype)
    Mp[:, :K] = M
    c, nt, j, lane, e = np.indices((NCH, NT, 2, 64, 4))
    q, c16 = lane // 16, lane % 16
    return Mp[16 * nt + c16, 32 * c + 16 * j + 4 * q + e].ravel()


def pack_pf(W):      # forward copy: N = rows, K = cols
    return pack_np(W)


def pack_pb(W):      # backward copy: K = rows, N = cols, operand [n][k] = W[k][n]
    return pack_np(np.ascontiguousarray(W.T))


# ------------------------------------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize("rows,cols", [(16, 32), (48, 96), (32, 48), (128, 256), (256, 256)])
def test_refresh_writes_the_documented_layout(rows, cols):
    from stnf import _native as N
    rs = np.random.RandomState(rows * 1000 + cols)
    off = 8                                     # the matrix does not start the flat buffer
    flat = rs.standard_normal(off + rows * cols + 4).astype(np.float32)
    W = flat[off:off + rows * cols].reshape(rows, cols)
    nf, nb = N.pack_f32_sizes(rows, cols)
    assert nf == pack_pf(W).size and nb == pack_pb(W).size
    d = T.dev()
    # NaN-filled: the refresh must write every entry, the zeros beyond K included
    pf = torch.full((nf,), float("nan"), device=d)
    pb = torch.full((nb,), float("nan"), device=d)
    N.f32_pack_refresh(torch.from_numpy(flat).to(d), N.make_bf16_shadow([(off, rows, cols, pf, pb)]))
    torch.cuda.synchronize()
    assert np.array_equal(pf.cpu().numpy(), pack_pf(W))
    assert np.array_equal(pb.cpu().numpy(), pack_pb(W))


# ------------------------------------------------------------------------------------------------ 2. / 3. steps
def _engine(hidden, B, pack, **kw):
    """TrainStep over a model with `hidden`; `pack`: with the packed copies, at any width the library takes (the
    engine's own default installs them only at the widths of its measured configurations)."""
    from stnf.engine import TrainStep
    base = "c2_b257" if hidden[0] == 256 else "default227"
    m = T.build_model(dict(cases.MODEL_CASES[base], hidden_dims=list(hidden)), dropout=0.1).train()
    eng = TrainStep(m, lr=1e-3, grad_clip=0.5, ema_decay=0.99, max_batch=B, seed=11, pack_weights=False, **kw)
    assert eng._whole_step and eng.uses_window and eng._pack_params is None
    if pack:
        eng._install_packed_copies()
        assert eng._pack_params is not None
    return eng


def _data(n, seed):
    rs = np.random.RandomState(seed)
    d = T.dev()
    return (torch.from_numpy(rs.uniform(0, 1, (n, 2)).astype(np.float32)).to(d),
            torch.from_numpy(rs.uniform(0, 1, (n,)).astype(np.float32)).to(d),
            torch.from_numpy(rs.standard_normal((n, 1)).astype(np.float32)).to(d))


@functools.lru_cache(maxsize=None)
def _three_steps(hidden, B, pack):
    """State after 3 one-call steps (stdadk_train_step_f32) on the same batches from the same state."""
    from stnf import _native as N
    eng = _engine(list(hidden), B, pack)
    coords, t, y = _data(3 * B, 100 + B)
    N.profile_enable(True)
    try:
        for i in range(3):
            eng.step(None, coords[i * B:(i + 1) * B], t[i * B:(i + 1) * B], y[i * B:(i + 1) * B])
        names = [k for k, _ in N.profile_collect()]
    finally:
        N.profile_enable(False)
    torch.cuda.synchronize()
    out = dict(loss=eng.loss_sum.clone(), grad=eng.grad.clone(), flat=eng.flat.clone(), m=eng.m.clone(),
               v=eng.v.clone(), ema=eng.ema.clone(), step=int(eng.step_dev.item()), names=names, copies=None)
    if pack:
        out["copies"] = [(o, h, hp, pf.clone(), pb.clone()) for o, h, hp, pf, pb in eng._pack_regions]
    return out


@pytest.mark.parametrize("B", [B_RAGGED, B_L1_TAIL, B_ROWS32, B_ROWS64])
@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(map(str, h)))
def test_steps_with_and_without_the_flag_are_equal(hidden, B):
    ref, got = _three_steps(tuple(hidden), B, False), _three_steps(tuple(hidden), B, True)
    assert ref["step"] == got["step"] == 3
    assert torch.isfinite(ref["flat"]).all()
    # the flag selects no other kernel: the same launches, and the one the batch size stands for among them
    assert got["names"] == ref["names"], (ref["names"], got["names"])
    assert KERNEL_OF[B] in ref["names"], ref["names"]
    for k in ("grad", "flat", "m", "v", "ema"):
        assert torch.equal(got[k], ref[k]), k
    l_ref, l_got = float(ref["loss"].item()), float(got["loss"].item())
    bound = loss_reorder_bound(B, ROWS_PER_WG[B])
    print(f"loss sum {l_got!r} against {l_ref!r}: relative difference {abs(l_got - l_ref) / l_ref:.3g}, bound {bound:.3g}")
    assert abs(l_got - l_ref) <= bound * l_ref


@pytest.mark.parametrize("B", [B_RAGGED, B_L1_TAIL])
@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(map(str, h)))
def test_optimiser_keeps_the_copies_current(hidden, B):
    got = _three_steps(tuple(hidden), B, True)
    flat = got["flat"].cpu().numpy()
    assert len(got["copies"]) == len(hidden) - 1
    for off, h, hp, pf, pb in got["copies"]:
        W = flat[off:off + h * hp].reshape(h, hp)
        assert np.array_equal(pf.cpu().numpy(), pack_pf(W)), (h, hp)
        assert np.array_equal(pb.cpu().numpy(), pack_pb(W)), (h, hp)


# ------------------------------------------------------------------------------------------------ 4. lifecycle
def _lifecycle(pack_weights, use_graph=False, B=256):
    from stnf.engine import TrainStep
    m = T.build_model(cases.MODEL_CASES["c2_b257"], dropout=0.1).train()
    eng = TrainStep(m, lr=1e-3, grad_clip=0.5, ema_decay=0.99, max_batch=B, seed=11, pack_weights=pack_weights,
                    use_graph=use_graph)
    assert (eng._pack_params is not None) == pack_weights       # [256, 256, 128]: the default installs the copies
    coords, t, y = _data(4 * B, 7)

    def step(i):
        eng.step(None, coords[i * B:(i + 1) * B], t[i * B:(i + 1) * B], y[i * B:(i + 1) * B])

    step(0)
    step(1)
    eng.swap_in_ema()
    eng.swap_in_ema()
    step(2)
    rs = np.random.RandomState(3)
    sd = {k: v + torch.from_numpy((0.01 * rs.standard_normal(tuple(v.shape))).astype(np.float32)).to(v.device)
          if v.dtype == torch.float32 and k.endswith("weight") else v for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    step(3)
    torch.cuda.synchronize()
    return eng.flat.clone(), eng.ema.clone()


def test_lifecycle_with_and_without_packed_weights():
    ref, got = _lifecycle(False), _lifecycle(True)
    assert torch.isfinite(ref[0]).all()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_graph_replay_equals_eager_with_packed_weights():
    ref, got = _lifecycle(True), _lifecycle(True, use_graph=True)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_swap_in_ema_refreshes_the_copies():
    """After the swap the copies hold the EMA weights (what a step under swapped weights would multiply by)."""
    B = 64
    eng = _engine([256, 256, 128], B, True)
    coords, t, y = _data(B, 5)
    eng.step(None, coords, t, y)
    eng.swap_in_ema()
    torch.cuda.synchronize()
    flat = eng.flat.cpu().numpy()
    for off, h, hp, pf, pb in eng._pack_regions:
        W = flat[off:off + h * hp].reshape(h, hp)
        assert np.array_equal(pf.cpu().numpy(), pack_pf(W)) and np.array_equal(pb.cpu().numpy(), pack_pb(W))


# ------------------------------------------------------------------------------------------------ 5. error paths
def _step_args(eng, B):
    from stnf import distributed as D
    coords, t, y = _data(B, 9)
    st = eng.state
    eng.step(None, coords, t, y)                    # builds the optimiser descriptor
    return (st.basis, st.desc), (coords, t, None, y, None, B, D.grad_scale(B, 1), eng.loss_sum, eng.ws)


def test_flag_with_bf16_is_an_argument_error():
    from stnf import _native as N
    eng = _engine([256, 256, 128], 64, True)
    (basis, desc), rest = _step_args(eng, 64)
    flat0 = eng.flat.clone()
    with pytest.raises(RuntimeError, match=r"code -1\)"):          # STDADK_E_ARG
        N.train_step(basis, desc, eng._pack_params, eng.grads_t, *rest,
                     eng.state.flags | N.FLAG_PACK_F32 | N.FLAG_BF16, eng._optim, seed=eng.seed)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat, flat0)             # refused before anything was enqueued


def test_misaligned_packed_pointer_is_an_alignment_error():
    from stnf import _native as N
    eng = _engine([256, 256, 128], 64, True)
    (basis, desc), rest = _step_args(eng, 64)
    flat0 = eng.flat.clone()
    for slot in ("W_bf16", "WT_bf16"):
        bad = N.MlpTensors.from_buffer_copy(eng._pack_params)
        getattr(bad, slot)[1] = getattr(bad, slot)[1] + 4        # PF / PB of layer 1 off by one float
        with pytest.raises(RuntimeError, match=r"code -3\)"):      # STDADK_E_ALIGN
            N.train_step(basis, desc, bad, eng.grads_t, *rest, eng.state.flags | N.FLAG_PACK_F32, eng._optim,
                         seed=eng.seed)
    # ... and in the table of stdadk_f32_pack_refresh
    off, h, hp, pf, pb = eng._pack_regions[0]
    with pytest.raises(RuntimeError, match=r"code -3\)"):
        N.f32_pack_refresh(eng.flat, N.make_bf16_shadow([(off, h, hp, pf[1:], pb)]))
    torch.cuda.synchronize()
    assert torch.equal(eng.flat, flat0)
