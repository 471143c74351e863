"""Training steps with GENERATED dropout masks -- the shipped configuration, dropout 0.1, and what bench.py times --
against float64.  Every other float64 test runs with dropout 0 or passes explicit masks, and every other dropout test
compares two GPU runs that share the mask code, so an error in the generated mask common to both cancels there: a
backward keyed differently from its forward, a mask that does not move with the step or the layer, a keep rate that
does not match the scale.  Here the reference gets its masks from oracle/dropout.py, the CPU restatement of the
contract in include/stdadk.h, which never calls the library; cases and comparison are tests/golden/dropout_cases.py
(tests/test_dropout_cases_cpu.py shows the comparison fails each of those errors).

Tolerances: the project's 1e-5 as test_gpu_mlp_shapes.py -- y max-abs over max(1, max|y|), loss relative, every gradient
tensor rel-L2 after orc.fit_kink_sides, parameters and EMA after a step with eps = test_gpu_round2._DP_EPS.  Every
test prints what it achieved.  Out of scope: bf16 operands (their reference, test_gpu_bf16.emulate, has no masks) and
learnable-knot / quantile steps, which share these epilogues.
"""
import numpy as np
import pytest
import torch

from golden import cases
from golden import dropout_cases as DC
from golden import shape_cases as SC
from oracle import dropout as drp
from oracle import stdadk_oracle as orc

import test_gpu_parity as T
import test_gpu_round2 as R2
from test_gpu_large_batch import _views

pytestmark = pytest.mark.gpu
TOL = DC.TOL

_REF = {}


def _inputs(e):
    if ("inputs", e) not in _REF:
        cfg = DC.config(e)
        _REF[("inputs", e)] = (cfg, SC.make_inputs(cfg), {k: v.astype(np.float64) for k, v in cases.make_state(cfg).items()})
    return _REF[("inputs", e)]


def _reference(e, seed, window, step=0):
    """The float64 step of an entry at its INITIAL parameters, computed once per (seed, step, row order)."""
    key = (e, seed, step, window)
    if key not in _REF:
        cfg, inp, params = _inputs(e)
        _REF[key] = DC.reference(cfg, inp, params, seed, step, window)
    return _REF[key]


def _dev_inputs(cfg, inp):
    X, coords, t, y = (torch.from_numpy(a).to(T.dev()) for a in inp)
    return (X if cfg["p"] else None), coords, t, y


def _model(cfg):
    m = T.build_model(cfg, dropout=cfg["dropout"])
    m.train()
    return m


def _oracle_keyed(m, cfg, by_model_key):
    """{oracle key: array}: the Dropout modules shift nn.Sequential's indices, cases.state_layout counts none."""
    names = [k for k, _ in m.named_parameters()]
    return {ko: by_model_key[km] for km, ko in zip(names, cases.make_state(cfg))}


def _cap(e):
    return DC.MAX_NEAR_KINK if e[1] == DC.SMALL_B else None


# ------------------------------------------------------------------ a. the mask itself, bit for bit
def _mlp_calls(m, cfg, feats):
    """run(seed, masks, dY) -> (y, gradients): stdadk_mlp_forward_f32 + backward_f32 on given features; dY a tensor,
    or a function of y."""
    from stnf import _native as N
    d = T.dev()
    B, Q = cfg["B"], cfg["output_dim"]
    desc = m._native_desc()
    ws = torch.empty(N.mlp_workspace_bytes(desc, B) // 4, device=d)

    def run(seed, masks, dY):
        yp = torch.empty(B, Q, device=d)
        N.mlp_forward(desc, m._native_tensors(), feats, B, yp, ws, True, seed, masks)
        grads = [torch.zeros_like(q) for q in m._param_list()]
        N.mlp_backward(desc, m._native_tensors(), m._pack(grads), feats, B, dY(yp) if callable(dY) else dY, ws, seed,
                       masks)
        return yp, grads
    return run


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["g_h40_24", "g_h320_72_q3"])
def test_generated_mask_equals_replica_bit_for_bit(name, p):
    """stdadk_mlp_forward_f32 / backward_f32 with seed s and generated masks == the same calls with the replica's
    masks passed as explicit uint8 arrays (the route test_dropout_masks_forward_backward pins to float64): y and
    every gradient torch.equal, for the three seeds.  Both routes run the per-layer kernels of mlp.hip here."""
    from stnf import _native as N
    cfg = dict(SC.SHAPE_CASES[name], B=197)
    X, coords, t, y = SC.make_inputs(cfg)
    d = T.dev()
    m = T.build_model(cfg, dropout=p)
    B, Q = cfg["B"], cfg["output_dim"]
    feats = m.build_features(*(torch.from_numpy(a).to(d) for a in (X, coords, t)))
    yd = torch.from_numpy(y).to(d)

    def mse_grad(yp):
        dY = torch.empty(B, Q, device=d)
        N.mse(yp, yd, 1.0 / (B * Q), dY, None)
        return dY

    run = _mlp_calls(m, cfg, feats)
    rows = np.arange(B)
    outs = []
    for seed in DC.SEEDS:
        mk = drp.keep_masks(seed, 0, rows, cfg["hidden_dims"], p)
        md = [torch.from_numpy(a.astype(np.uint8)).to(d) for a in mk]
        y_gen, g_gen = run(seed, None, mse_grad)
        y_rep, g_rep = run(seed, md, mse_grad)
        kept = sum(int(a.sum()) for a in mk) / sum(a.size for a in mk)
        same = torch.equal(y_gen, y_rep) and all(torch.equal(a, b) for a, b in zip(g_gen, g_rep))
        print(f"{name} p={p:g} seed={seed}: kept {kept:.5f}; generated == replica masks: {same}; max |dy| "
              f"{(y_gen - y_rep).abs().max().item():.2e}")
        assert torch.equal(y_gen, y_rep), seed
        for k, (a, b) in enumerate(zip(g_gen, g_rep)):
            assert torch.equal(a, b), (seed, k)
        outs.append(y_gen)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


def test_generated_mask_equals_replica_bit_for_bit_h256_256_128():
    """The same for a [256, 256, 128] model.  The fused tail takes such widths when no masks are passed, so the
    generated route runs tail_body.h (ln_fwd_rows / ln_bwd_rows, CC = 4 and CC = 2) and the explicit one the per-layer
    kernels: two GEMMs that round differently.  To keep torch.equal meaningful the network is made EXACT: integer
    features, weights and dY in {-1, 0, 1}, no LayerNorm, p = 0.5 (scale 2), so every sum is an integer below 2^23
    and no summation order rounds.  Then generated == explicit == the float64 oracle with the replica's masks, bit
    for bit, on y and every gradient."""
    p = 0.5
    cfg = dict(SC.SHAPE_CASES["w_depth1"], hidden_dims=[256, 256, 128], layernorm=False, seed=131, B=197)
    X, coords, t, _ = SC.make_inputs(cfg)
    d = T.dev()
    m = T.build_model(cfg, dropout=p)
    B, nh = cfg["B"], len(cfg["hidden_dims"])
    rs = np.random.RandomState(cfg["seed"])
    params = {k: rs.randint(-1, 2, v.shape).astype(np.float64) for k, v in cases.make_state(cfg).items()}
    with torch.no_grad():
        for q, v in zip(m.parameters(), params.values()):
            q.copy_(torch.from_numpy(v.astype(np.float32)))
    feats = m.build_features(*(torch.from_numpy(a).to(d) for a in (X, coords, t)))
    D = params["mlp.0.weight"].shape[1]
    f_int = rs.randint(-1, 2, (B, D)).astype(np.float64)
    feats.zero_()
    feats[:, :D] = torch.from_numpy(f_int.astype(np.float32)).to(d)
    dy = rs.randint(-1, 2, (B, 1)).astype(np.float64)
    dY = torch.from_numpy(dy.astype(np.float32)).to(d)
    run = _mlp_calls(m, cfg, feats)
    rows = np.arange(B)
    for seed in DC.SEEDS:
        mk = drp.keep_masks(seed, 0, rows, cfg["hidden_dims"], p)
        yo, cache = orc.mlp_forward(f_int, params, nh, False, drop_masks=mk, drop_p=p)
        go = orc.mlp_backward(dy, cache, params, nh, False)
        big = max([np.abs(yo).max()] + [np.abs(c[3]).max() * 2 for c in cache[:-1]] + [np.abs(g).max() for g in go.values()])
        assert big < 2 ** 23, big                                     # exact in float32 whatever the order
        md = [torch.from_numpy(a.astype(np.uint8)).to(d) for a in mk]
        y_gen, g_gen = run(seed, None, dY)
        y_rep, g_rep = run(seed, md, dY)
        print(f"h256_256_128 exact p={p:g} seed={seed}: largest integer {big:.0f}; max |y_generated - y_explicit| "
              f"{(y_gen - y_rep).abs().max().item():.1e}, max |y_generated - y_float64| "
              f"{np.abs(y_gen.cpu().numpy() - yo).max():.1e}")
        assert torch.equal(y_gen, y_rep) and np.array_equal(y_gen.cpu().numpy().astype(np.float64), yo), seed
        for k, a, b in zip(params, g_gen, g_rep):
            assert torch.equal(a, b), (seed, k)
            assert np.array_equal(a.cpu().numpy().astype(np.float64), go[k]), (seed, k)


# ------------------------------------------------------------------ b. module forward + backward
B_PARAMS = [(e, "auto") for e in DC.ENTRIES] + [(e, "dense") for e in DC.ENTRIES if e[0] in DC.WINDOW_CASES
                                                and e[1] == DC.SMALL_B]


def _module_case(e, path):
    from stnf import _native as N
    cfg, inp, _ = _inputs(e)
    m = _model(cfg)
    m.force_dense_path = path == "dense"
    st = m._step_state(T.dev(), force_dense=m.force_dense_path)
    window = N.step_uses_window(st.basis, st.desc, st.flags)
    assert window == (path == "auto" and e[0] in DC.WINDOW_CASES)
    k = DC.ENTRIES.index(e)
    torch.manual_seed(k)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())           # what the module is about to draw
    torch.manual_seed(k)
    X, coords, t, y = _dev_inputs(cfg, inp)
    yp = m(X, coords, t)
    loss = torch.nn.MSELoss()(yp, y)
    loss.backward()
    got = {km: q.grad.cpu().numpy() for km, q in m.named_parameters()}
    return yp.detach().cpu().numpy(), loss.item(), _oracle_keyed(m, cfg, got), _reference(e, seed, window)


@pytest.mark.parametrize("e,path", B_PARAMS, ids=lambda v: DC.entry_id(v) if isinstance(v, tuple) else v)
def test_module_forward_backward_against_float64(e, path):
    print(f"{DC.entry_id(e)} [{path}]:")
    got_y, got_loss, got_g, ref = _module_case(e, path)
    DC.compare(got_y, got_loss, got_g, ref, max_alts=_cap(e))


@pytest.mark.parametrize("group", ["1", "2"])
def test_module_with_grouped_layer0(group, monkeypatch):
    """One and two observations per wave in the layer-0 window forward: the epilogue's row is the sorted row of each."""
    monkeypatch.setenv("STDADK_L1_GROUP", group)
    e = DC.ENTRIES[1]
    print(f"{DC.entry_id(e)} STDADK_L1_GROUP={group}:")
    got_y, got_loss, got_g, ref = _module_case(e, "auto")
    DC.compare(got_y, got_loss, got_g, ref, max_alts=_cap(e))


# ------------------------------------------------------------------ c. TrainStep, the path bench.py times
def _train_steps(e, how="step", use_graph=False):
    """DC.STEPS consecutive one-call steps; each step's loss and gradients against float64 at that step's own
    pre-step parameters with the replica's masks of step 0, 1, 2; parameters and EMA after the first."""
    from stnf.engine import TrainStep
    cfg, inp, params0 = _inputs(e)
    window = e[0] in DC.WINDOW_CASES
    seed = DC.entry_seed(e)
    B = cfg["B"]
    go0 = _reference(e, seed, window)[2]
    clip = DC.CLIP_OF_NORM * float(np.sqrt(sum(float((g * g).sum()) for g in go0.values())))
    o = cases.OPT
    assert DC.ADAM_EPS == R2._DP_EPS
    m = _model(cfg)
    eng = TrainStep(m, lr=o["lr"], weight_decay=o["weight_decay"], betas=o["betas"], eps=DC.ADAM_EPS, grad_clip=clip,
                    ema_decay=o["ema_decay"], max_batch=B, seed=seed, use_graph=use_graph)
    assert eng.uses_window == window and eng._whole_step and eng.seed == seed
    X, coords, t, y = _dev_inputs(cfg, inp)
    idx = torch.arange(B, device=T.dev())
    worst = dict(loss=0.0, grad=0.0, flipped=0, near=0)
    for s in range(DC.STEPS):
        torch.cuda.synchronize()
        if s == 0:
            ref = _reference(e, seed, window)
        else:
            pre = _oracle_keyed(m, cfg, _views(eng, m, eng.flat))
            ref = DC.reference(cfg, inp, pre, seed, s, window)
        if how == "step":
            eng.step(X, coords, t, y)
        else:
            eng.step_indexed(coords, t, y, idx, X_all=X, next_idx=idx if s + 1 < DC.STEPS else None)
            if window and s + 1 < DC.STEPS:
                assert eng._prepared is not None and eng._prepared.inline
        loss = eng.mean_loss()
        assert int(eng.step_dev.item()) == s + 1
        print(f"{DC.entry_id(e)} {how}{' graph' if use_graph else ''} step {s}:")
        # the near-kink COUNT is capped where the reference is fixed (step 0, tests/test_dropout_cases_cpu.py); at the
        # later steps the reference stands at the parameters this run has reached, so the cap is on the units the
        # fit may move
        r = DC.compare(None, loss, _oracle_keyed(m, cfg, _views(eng, m, eng.grad)), ref,
                       max_alts=_cap(e) if s == 0 else None)
        assert _cap(e) is None or len(r["flipped"]) <= DC.MAX_NEAR_KINK, r["flipped"]
        worst = dict(loss=max(worst["loss"], r["loss"]), grad=max(worst["grad"], r["worst"]),
                     flipped=worst["flipped"] + len(r["flipped"]), near=worst["near"] + r["near"])
        if s == 0:
            params = {k: v.copy() for k, v in params0.items()}
            mm = {k: np.zeros_like(v) for k, v in params.items()}
            vv = {k: np.zeros_like(v) for k, v in params.items()}
            sh = {k: v.copy() for k, v in params.items()}
            coef = orc.adamw_ema_step(params, r["adjusted"], mm, vv, sh, 1, o["lr"], o["weight_decay"], o["betas"],
                                      DC.ADAM_EPS, clip, o["ema_decay"])
            assert coef < 0.6
            p_got = _oracle_keyed(m, cfg, _views(eng, m, eng.flat))
            e_got = _oracle_keyed(m, cfg, _views(eng, m, eng.ema))
            ep = {k: T.rel_l2(p_got[k], params[k]) for k in params}
            ee = {k: T.rel_l2(e_got[k], sh[k]) for k in params}
            print(f"    after the step: parameters worst rel-L2 {max(ep.values()):.2e} ({max(ep, key=ep.get)}), EMA "
                  f"{max(ee.values()):.2e}")
            for k in params:
                assert ep[k] <= TOL, (k, ep[k])
                assert ee[k] <= TOL, (k, ee[k])
    print(f"{DC.entry_id(e)} {how}: worst over {DC.STEPS} steps: loss {worst['loss']:.2e}, gradient {worst['grad']:.2e}; "
          f"{worst['near']} near-kink units, {worst['flipped']} flipped")
    return eng.flat.clone()


@pytest.mark.parametrize("e", DC.ENTRIES, ids=DC.entry_id)
def test_train_steps_against_float64(e):
    _train_steps(e)


def test_step_indexed_with_the_next_batch_announced(monkeypatch):
    """The next batch binned inside the weight-gradient launch (default) and inside the optimiser launch
    (STDADK_BIN_IN=adam): the step counter advances where the masks expect it, and both end in equal parameters."""
    e = DC.ENTRIES[1]
    monkeypatch.delenv("STDADK_BIN_IN", raising=False)
    a = _train_steps(e, how="step_indexed")
    monkeypatch.setenv("STDADK_BIN_IN", "adam")
    b = _train_steps(e, how="step_indexed")
    assert torch.equal(a, b)


def test_graph_replay_reads_the_advancing_step():
    """use_graph=True: eager first step, capture, replay -- a replay must read step_dev, not a captured constant."""
    _train_steps(DC.ENTRIES[3], use_graph=True)


# ------------------------------------------------------------------ d. ranks
def test_ranks_draw_their_own_masks():
    """Ranks 0 and 1 of 2 on the same rows (the engine's virtual-rank mode): each matches float64 with the replica's
    masks under _rank_seed(base, rank), and the two differ."""
    from stnf.engine import TrainStep, _rank_seed
    e = DC.ENTRIES[DC.RANK_ENTRY]
    cfg, inp, _ = _inputs(e)
    window = e[0] in DC.WINDOW_CASES
    B, Q = cfg["B"], cfg["output_dim"]
    X, coords, t, y = _dev_inputs(cfg, inp)
    grads = []
    for rank in (0, 1):
        m = _model(cfg)
        eng = TrainStep(m, max_batch=B, world_size=2, seed=DC.RANK_BASE_SEED)
        eng.set_virtual_rank(rank)
        seed = _rank_seed(DC.RANK_BASE_SEED, rank)
        assert eng.seed == seed == (DC.RANK_BASE_SEED + 0xD1B54A32D192ED03 * rank) % 2 ** 64 and eng.uses_window == window
        eng._enqueue_grads(X, coords, t.view(-1), y, B, B)
        loss = eng.loss_sum.item() / (B * Q)
        print(f"{DC.entry_id(e)} rank {rank} of 2:")
        DC.compare(None, loss, _oracle_keyed(m, cfg, _views(eng, m, eng.grad)), _reference(e, seed, window),
                   max_alts=_cap(e))
        grads.append(eng.grad.clone())
    assert not torch.equal(grads[0], grads[1])
    m0, m1 = (DC.masks(cfg, _rank_seed(DC.RANK_BASE_SEED, r), 0, np.arange(B)) for r in (0, 1))
    assert all((a != b).mean() > 0.1 for a, b in zip(m0, m1))
