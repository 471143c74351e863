"""Launch-chain guard of the step host code (CPU, no GPU): which kernels every library call enqueues, and in which order,
for every branch of the code that turns one call into a chain of launches (st-dadk_amd/csrc/mlp.hip).  A change of the
host code that moves, drops, adds or re-shapes a launch shows here before anything runs on a device.

How (as tests/test_engine_call_trace.py): with STDADK_DRY_RUN=1 every entry point validates and plans but launches
nothing; with the profiler on (stdadk_profile_enable) the dry run still records the NAME of every launch it skips, and
stdadk_profile_collect lists them.  The names of the stand-alone GEMMs carry their shapes and split counts.  This file is
its own driver: started as a script in a child process (stnf._native reads the variable at import) it runs every case
and prints one JSON record {case: [kernel names]}, which the tests compare with tests/golden/launch_chains.json.

The fixture was recorded from the host code as it stood BEFORE the stages of a step handed their launches on by value
(only the dry-run log added): it pins that order.  `python tests/test_launch_chains_cpu.py` prints the record of the
code at hand for a comparison by eye; re-record the fixture only for a change that is meant to alter a chain.

tests/test_gpu_launch_chains.py runs GPU_CASES for real and checks that the profiled launches carry the same names."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_chains.json")
ENV_SWITCHES = ("STDADK_DW_FIN", "STDADK_BIN_IN", "STDADK_NO_DW_ALL", "STDADK_NO_DENSE0_TAIL", "STDADK_NO_L1_TAIL",
                "STDADK_NO_TAIL_FWD_BWD", "STDADK_NO_FUSED_TAIL", "STDADK_TAIL_ROWS", "STNF_FUSED_KNOT_STEP",
                "STNF_NO_PACK_WEIGHTS", "STNF_NO_INLINE_PREP")
# the cases a real device repeats (64 rows each): window one-call step, materialising one-call step, learnable fused
# step on the window path, split train_fwd_bwd with y_pred
GPU_CASES = ("window/b64", "dense/d0", "knots/fused_window", "doors/fwd_bwd_ypred_window")


class _FakeStream:
    """An auxiliary stream handle for a dry run: any non-null value different from the main stream (never dereferenced)."""
    cuda_stream = 0x1000


def cases(dev="cpu"):
    """{name: thunk}; every thunk makes the library calls of its case (models and engines are built on first use)."""
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    from stnf import _native as N
    from stnf.engine import TrainStep
    from stnf.models import STInterpMLP

    def model(hidden, window=False, knots=(25, 81), **kw):
        torch.manual_seed(0)
        m = STInterpMLP(p=kw.pop("p", 0), k_spatial_centers=list(knots), k_temporal_centers=[10, 15],
                        hidden_dims=list(hidden), dropout=0.1, layernorm=True, **kw).train()
        m.force_window_path = bool(window)
        return m.to(dev)

    def engine(m, B=64, **kw):
        eng = TrainStep(m, max_batch=B, ema_decay=0.99, seed=7, **kw)
        assert eng.uses_window == bool(m.force_window_path), (eng.uses_window, m.force_window_path)
        return eng

    def data(n, q=1, p=0):
        g = torch.Generator().manual_seed(1)
        c, t, y = torch.rand(n, 2, generator=g), torch.rand(n, generator=g), torch.randn(n, q, generator=g)
        X = torch.randn(n, p, generator=g) if p else None
        return (X.to(dev) if p else None), c.to(dev), t.to(dev), y.to(dev)

    memo = {}

    def once(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]

    def with_env(thunk, **env):
        def run():
            for k, v in env.items():
                os.environ[k] = v
            try:
                return thunk()
            finally:
                for k in env:
                    del os.environ[k]
        return run

    def step(key, make_engine, B=64, q=1, p=0):
        """One optimisation step of an engine on B rows, as TrainStep enqueues it."""
        def run():
            eng = once(key, make_engine)
            X, c, t, y = once(("data", B, q, p), lambda: data(B, q, p))
            N.profile_enable(True)          # (drops what building the engine launched: operand copies)
            eng._enqueue(X, c, t, y, B, B)
        return run

    WIN, DENSE = (128, 64), (64, 64)
    out = {}

    # ---- one-call step, fixed knots, window path
    win = lambda **kw: (lambda: engine(model(WIN, window=True), **kw))
    out["window/b64"] = step("win", win())
    out["window/b8192"] = step("win8192", win(B=8192), B=8192)
    for mode in "012":
        out[f"window/dw_fin{mode}"] = with_env(step("win", win()), STDADK_DW_FIN=mode)
    out["window/b49152_narrow"] = step("win_narrow", lambda: engine(model((128, 16), window=True), B=49152), B=49152)
    out["window/no_dw_all"] = with_env(step("win", win()), STDADK_NO_DW_ALL="1")
    out["window/no_l1_tail"] = with_env(step("win", win()), STDADK_NO_L1_TAIL="1")
    out["window/no_tail_fwd_bwd"] = with_env(step("win", win()), STDADK_NO_TAIL_FWD_BWD="1")
    out["window/noclip"] = step("win_noclip", win(grad_clip=0))
    out["window/sparsity"] = step("win_sparse", win(sparsity_penalty_type="sparse_group"))
    out["window/bf16"] = step("win_bf16", win(dtype="bf16"))

    def packed():
        eng = engine(model((256, 128), window=True))
        assert eng._pack_params is not None
        return eng
    out["window/packed"] = step("win_packed", packed)
    out["window/covariates_q5"] = step("win_q5", lambda: engine(
        model(WIN, window=True, p=3, output_dim=5), loss="pinball", quantile_levels=[0.05, 0.25, 0.5, 0.75, 0.95]),
        q=5, p=3)

    # ---- one-call step, materialising path
    dense = lambda hidden=DENSE, **kw: (lambda: engine(model(hidden, **kw)))
    out["dense/d0"] = step("dense", dense())
    out["dense/no_dense0_tail"] = with_env(step("dense", dense()), STDADK_NO_DENSE0_TAIL="1")
    out["dense/wide_input"] = step("dense_wide", dense(knots=(25, 81, 400)))       # D = 531 > TAIL_D0_MAX
    out["dense/refused_widths"] = step("dense_generic", dense(hidden=(40, 24)))
    out["dense/noclip"] = step("dense_noclip", lambda: engine(model(DENSE), grad_clip=0))
    out["dense/bf16"] = step("dense_bf16", lambda: engine(model(DENSE), dtype="bf16"))

    def dense_w0_out_in():
        # the engine always stores W0 (in,out); the (out,in) layout through the door itself (a dry run reads no weight)
        eng = once("dense", dense())
        X, c, t, y = once(("data", 64, 1, 0), lambda: data(64))
        eng._enqueue(X, c, t, y, 64, 64)                 # (builds eng._optim)
        N.profile_enable(True)                           # drop that step's records
        st = eng.state
        N.train_step(st.basis, st.desc, st.params, eng.grads_t, c, t, None, y, None, 64, 1.0 / 64, eng.loss_sum, eng.ws,
                     st.flags & ~N.FLAG_W0_T, eng._optim, seed=7)
    out["dense/w0_out_in"] = dense_w0_out_in

    # ---- one-call step that announces its next batch
    def step_next(B, nB, overlap=False):
        def run():
            eng = once(("win_next", max(B, nB)), win(B=max(B, nB)))
            X, c, t, y = once(("data", max(B, nB), 1, 0), lambda: data(max(B, nB)))
            idx, nidx = torch.arange(B - 1, -1, -1, device=dev), torch.arange(nB, device=dev)
            if overlap:
                big = torch.empty(2 * eng.ws.numel() + 8, device=dev)
                ws, ws2 = big[:eng.ws.numel()], big[4:4 + eng.ws.numel()]
            else:
                ws, ws2 = eng.ws, once(("ws2", max(B, nB)), lambda: torch.empty_like(eng.ws))
            N.profile_enable(True)
            return eng._enqueue(X, c, t, y, B, B, idx=idx, ws=ws, nxt=(nidx, ws2))
        return run
    out["next/in_dw"] = step_next(64, 64)
    out["next/in_adam"] = with_env(step_next(64, 64), STDADK_BIN_IN="adam")
    out["next/overlapping_workspaces"] = step_next(64, 64, overlap=True)
    out["next/too_large"] = step_next(64, 6000)

    # ---- learnable knots
    learn = lambda hidden, window=False, **kw: (lambda: engine(model(hidden, window=window, spatial_learnable=True), **kw))
    out["knots/split_window"] = step("learn_split_win", learn(WIN, True))
    out["knots/split_dense"] = step("learn_split_dense", learn(DENSE))
    out["knots/fused_window"] = step("learn_fused_win", learn(WIN, True, fused_knot_step=True))
    for mode in "012":
        out[f"knots/fused_window_dw_fin{mode}"] = with_env(step("learn_fused_win", learn(WIN, True, fused_knot_step=True)),
                                                           STDADK_DW_FIN=mode)
    out["knots/fused_window_no_dw_all"] = with_env(step("learn_fused_win", learn(WIN, True, fused_knot_step=True)),
                                                   STDADK_NO_DW_ALL="1")
    out["knots/fused_window_noclip"] = step("learn_fused_win_noclip", learn(WIN, True, fused_knot_step=True, grad_clip=0))
    out["knots/fused_dense"] = step("learn_fused_dense", learn(DENSE, fused_knot_step=True))

    def scattered(**kw):
        def make():
            g = torch.Generator().manual_seed(3)
            pts = torch.rand(600, 2, generator=g).numpy()
            m = model(WIN, window=True, knots=(64, 256), spatial_learnable=True, spatial_init_method="random_site",
                      train_coords=pts)
            eng = engine(m, **kw)
            assert eng.state.flags & N.FLAG_SCATTERED
            return eng
        return make
    out["knots/scattered_window_split"] = step("scat_split", scattered())
    out["knots/scattered_window_fused"] = step("scat_fused", scattered(fused_knot_step=True))

    # ---- the split doors, called directly with the descriptors of a split-path engine
    def door(key, make_engine, call, B=64):
        def run():
            eng = once(key, make_engine)
            X, c, t, y = once(("data", B, 1, 0), lambda: data(B))
            N.profile_enable(True)
            return call(eng, eng.state, c, t, y, B)
        return run

    split = lambda hidden, window=False, **kw: (lambda: engine(model(hidden, window=window), world_size=2, **kw))

    def fwd_bwd(y_pred=False, aux=False):
        def call(eng, st, c, t, y, B):
            yp = once(("yp", B), lambda: torch.empty(B, 1, device=dev)) if y_pred else None
            N.train_fwd_bwd(st.basis, st.desc, st.params, eng.grads_t, c, t, None, y, B, 1.0 / B, eng.loss_sum, yp, eng.ws,
                            st.flags, seed=7, step_dev=eng.step_dev, aux_stream=_FakeStream() if aux else None)
        return call

    def two_calls(eng, st, c, t, y, B):
        yp = once(("yp", B), lambda: torch.empty(B, 1, device=dev))
        N.forward(st.basis, st.desc, st.params, c, t, None, B, yp, eng.ws, st.flags, training=True, seed=7,
                  step_dev=eng.step_dev)
        N.backward(st.basis, st.desc, st.params, eng.grads_t, B, yp, eng.ws, st.flags, seed=7, step_dev=eng.step_dev)

    out["doors/fwd_bwd_ypred_window"] = door("split_win", split(WIN, True), fwd_bwd(y_pred=True))
    out["doors/fwd_bwd_ypred_dense"] = door("split_dense", split(DENSE), fwd_bwd(y_pred=True))
    out["doors/fwd_bwd_window"] = door("split_win", split(WIN, True), fwd_bwd())
    out["doors/forward_backward_window"] = door("split_win", split(WIN, True), two_calls)
    out["doors/forward_backward_dense"] = door("split_dense", split(DENSE), two_calls)
    out["doors/forward_backward_dense_bf16"] = door("split_dense_bf16", split(DENSE, dtype="bf16"), two_calls)
    out["doors/forward_backward_refused_widths"] = door("split_generic", split((40, 24)), two_calls)
    if dev == "cpu":        # (a handle that is no stream: dry run only)
        out["doors/aux_stream_window"] = door("split_win", split(WIN, True), fwd_bwd(aux=True))
        out["doors/aux_stream_window_b8192"] = door("split_win8192", split(WIN, True, B=8192), fwd_bwd(aux=True), B=8192)
        out["doors/aux_stream_window_refused_widths"] = door("split_win_generic", split((128, 40), True), fwd_bwd(aux=True))
        out["doors/aux_stream_dense"] = door("split_dense", split(DENSE), fwd_bwd(aux=True))
    out["doors/fwd_bwd_window_refused_widths"] = door("split_win_generic", split((128, 40), True), fwd_bwd())

    def knot_backward(eng, st, c, t, y, B):
        N.knot_backward(st.basis, st.desc, st.params, c, B, eng.ws, st.flags, eng._knot_train_desc(B), eng.g_centers,
                        eng.g_log_bw, eng.loss_sum)
    out["doors/knot_backward_window"] = door("learn_split_win", learn(WIN, True), knot_backward)
    out["doors/knot_backward_dense"] = door("learn_split_dense", learn(DENSE), knot_backward)

    def mlp(masks):
        def call(eng, st, c, t, y, B):
            d = st.desc
            feats = once(("feats", B, d.in_dim), lambda: torch.empty(B, (d.in_dim + 31) // 32 * 32, device=dev))
            ws = once(("mlp_ws", id(eng)), lambda: torch.empty(N.mlp_workspace_bytes(d, B) // 4, device=dev))
            yp = once(("yp", B), lambda: torch.empty(B, 1, device=dev))
            mk = [torch.ones(B, d.hidden[l], dtype=torch.uint8, device=dev) for l in range(d.n_hidden)] if masks else None
            N.mlp_forward(d, st.params, feats, B, yp, ws, True, seed=7, masks=mk)
            N.mlp_backward(d, st.params, eng.grads_t, feats, B, yp, ws, seed=7, masks=mk)
        return call
    out["doors/mlp"] = door("split_dense", split(DENSE), mlp(False))
    out["doors/mlp_masks"] = door("split_dense", split(DENSE), mlp(True))
    out["doors/mlp_refused_widths"] = door("split_generic", split((40, 24)), mlp(False))

    def eval_indexed(eng, st, c, t, y, B):
        idx = torch.arange(B - 1, -1, -1, device=dev)
        ws = once(("eval_ws", id(eng)), lambda: torch.empty(N.eval_workspace_bytes(st.basis, st.desc, B, st.flags) // 4,
                                                            device=dev))
        acc = once("acc", lambda: torch.zeros(N.EVAL_SLOTS, dtype=torch.float64, device=dev))
        yp = once(("yp", B), lambda: torch.empty(B, 1, device=dev))
        N.eval_indexed(st.basis, st.desc, st.params, c, t, None, y, idx, None, 0, 1.0, acc, yp, ws, st.flags)
    out["doors/eval_window"] = door("split_win", split(WIN, True), eval_indexed)
    out["doors/eval_dense"] = door("split_dense", split(DENSE), eval_indexed)
    return out


def record(dev="cpu", only=None):
    """{case: [kernel names in launch order]} of the cases (all, or `only`)."""
    todo = cases(dev)
    from stnf import _native as N
    rec = {}
    for name in (only or sorted(todo)):
        N.profile_enable(True)
        try:
            todo[name]()
            rec[name] = [k for k, _ in N.profile_collect()]
        finally:
            N.profile_enable(False)
    return rec


def expected():
    with open(FIXTURE) as f:
        return json.load(f)


_cache = {}


def _recorded():
    if "rec" not in _cache:
        env = dict(os.environ, STDADK_DRY_RUN="1")
        for k in ENV_SWITCHES:
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        line = [l for l in r.stdout.splitlines() if l.startswith("RECORD ")][-1]
        _cache["rec"] = json.loads(line[len("RECORD "):])
    return _cache["rec"]


def test_every_case_is_recorded():
    assert sorted(_recorded()) == sorted(expected())
    assert set(GPU_CASES) <= set(expected())


@pytest.mark.parametrize("name", sorted(expected()) if os.path.exists(FIXTURE) else [])
def test_launch_chain(name):
    """Names, order, and the shapes / split counts the GEMM names carry."""
    got, want = _recorded()[name], expected()[name]
    assert want, name                    # no case records nothing
    assert got == want, (name, got, want)


if __name__ == "__main__":
    print("RECORD " + json.dumps(record(), sort_keys=True))
    sys.exit(0)
