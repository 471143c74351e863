"""The one-call delta step (stdadk_train_step_delta_f32, TrainStep(fused_delta_step=...)) on the host: which library
calls a step makes, when the engine takes the path, what the door refuses, and which kernels the call enqueues next to
the same model with a standard head of the same Q on the one-call door that exists without the head (CPU, no GPU).

How (as tests/test_knot_step_cpu.py and tests/test_launch_chains_cpu.py): with STDADK_DRY_RUN=1 every entry point of
libstdadk validates and plans but launches nothing, TrainStep runs on host tensors, and with the profiler on the dry run
records the name of every launch it skips.  This file is its own driver: started as a script in a child process
(stnf._native reads the variable at import) it prints one JSON record -- the entry points called per step, the error
text of every refused call, and {case: [kernel names]} -- which the tests compare with what the issue of the door
specifies and with tests/golden/launch_chains_delta.json.  `python tests/test_delta_step_cpu.py` prints the record of
the code at hand.

tests/test_gpu_delta_step.py runs GPU_CASES for real and checks that the profiled launches carry the same names."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_chains_delta.json")
B = 64
TAUS5 = [0.05, 0.25, 0.5, 0.75, 0.95]
DOOR = "train_step_delta_f32"
SPLIT_FIXED = ["delta_head_f32", "train_fwd_bwd_f32", "delta_head_backward_f32", "sumsq_f32", "adamw_ema_f32"]
SPLIT_LEARN = ["delta_head_f32", "train_fwd_bwd_f32", "delta_head_backward_f32", "knot_backward_f32", "sumsq2_f32",
               "adamw_ema2_f32"]
ENV_SWITCHES = ("STDADK_DW_FIN", "STDADK_BIN_IN", "STDADK_NO_DW_ALL", "STDADK_NO_FUSED_TAIL", "STNF_FUSED_KNOT_STEP",
                "STNF_FUSED_DELTA_STEP", "STNF_NO_PACK_WEIGHTS", "STNF_NO_INLINE_PREP")
GPU_CASES = ("delta/fixed_window", "delta/learn_window")
WIN, DENSE = (128, 64), (64, 64)


def _paths():
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _model(hidden, window, learn, delta, dev="cpu"):
    import torch
    from stnf.models import STInterpMLP
    torch.manual_seed(0)
    m = STInterpMLP(p=0, k_spatial_centers=[25, 81], k_temporal_centers=[10, 15], hidden_dims=list(hidden), dropout=0.1,
                    layernorm=True, output_dim=5, use_delta_reparameterization=delta, spatial_learnable=learn).train()
    m.force_window_path = bool(window)
    return m.to(dev)


def _engine(m, rows=B, **kw):
    from stnf.engine import TrainStep
    delta = m._has_delta
    eng = TrainStep(m, max_batch=rows, ema_decay=0.99, seed=7, loss="pinball", quantile_levels=TAUS5,
                    non_crossing_lambda=1.0 if delta else 0.0, non_crossing_weight=0.0 if delta else 0.5, **kw)
    assert eng.uses_window == bool(m.force_window_path)
    return eng


def _data(n, dev="cpu"):
    import torch
    g = torch.Generator().manual_seed(1)
    return (torch.rand(n, 2, generator=g).to(dev), torch.rand(n, generator=g).to(dev),
            torch.randn(n, 1, generator=g).to(dev))


# ------------------------------------------------------------------------------------------------ launch chains
def chain_cases(dev="cpu"):
    """{name: thunk}: "delta/<case>" is the fused delta step, "twin/<case>" the same model with a standard head of the
    same Q on today's one-call door (train_step for fixed knots, train_step_knots for learnable ones)."""
    _paths()
    from stnf import _native as N
    memo = {}

    def once(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]

    def step(delta, hidden, window, learn, rows=257, env=None, **kw):
        def run():
            for k, v in (env or {}).items():
                os.environ[k] = v
            try:
                key = (delta, hidden, window, learn, rows, tuple(sorted(kw.items())))
                if delta:
                    kw2 = dict(kw, fused_delta_step=True)
                else:
                    kw2 = dict(kw, fused_knot_step=True) if learn else dict(kw)
                eng = once(key, lambda: _engine(_model(hidden, window, learn, delta, dev), rows, **kw2))
                assert bool(eng._delta_step) == bool(delta)
                c, t, y = once(("data", rows), lambda: _data(rows, dev))
                N.profile_enable(True)        # (drops what building the engine launched)
                eng._enqueue(None, c, t, y, rows, rows)
            finally:
                for k in (env or {}):
                    del os.environ[k]
        return run

    out = {}
    for who, delta in (("delta", True), ("twin", False)):
        out[f"{who}/fixed_window"] = step(delta, WIN, True, False, rows=B)
        for mode in "012":
            out[f"{who}/fixed_window_dw_fin{mode}"] = step(delta, WIN, True, False, env={"STDADK_DW_FIN": mode})
        out[f"{who}/fixed_dense"] = step(delta, DENSE, False, False)
        out[f"{who}/learn_window"] = step(delta, WIN, True, True, rows=B)
        out[f"{who}/learn_dense"] = step(delta, DENSE, False, True)
        out[f"{who}/fixed_window_noclip"] = step(delta, WIN, True, False, grad_clip=0)
        out[f"{who}/learn_window_noclip"] = step(delta, WIN, True, True, grad_clip=0)
        out[f"{who}/fixed_window_sparsity"] = step(delta, WIN, True, False, sparsity_penalty_type="sparse_group")
        out[f"{who}/fixed_window_refused_widths"] = step(delta, (128, 40), True, False)
    return out


def record_chains(dev="cpu", only=None):
    """{case: [kernel names in launch order]} of the cases (all, or `only`)."""
    todo = chain_cases(dev)
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


def expected_chains():
    with open(FIXTURE) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ call traces, refusals
def _record_calls():
    _paths()
    import torch
    from stnf import _native as N
    from stnf import training as T
    from stnf.engine import TrainStep

    real = N.lib()
    log = []

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name in ("stdadk_last_error", "stdadk_abi_version"):
                return fn

            def call(*args):
                log.append(name.replace("stdadk_", ""))
                return fn(*args)
            return call

    proxy = Proxy()
    N.lib = lambda: proxy
    n = 4 * B
    coords, t, y = _data(n)

    def names(fn):
        del log[:]
        out = fn()
        return {"calls": list(log), "ret": out}

    def one(eng):
        return names(lambda: eng.step(None, coords[:B], t[:B], y[:B]))

    rec = {}
    for learn in (False, True):
        tag = "learn" if learn else "fixed"
        eng = _engine(_model(WIN, True, learn, True), fused_delta_step=True)
        rec[f"fused_{tag}"] = [one(eng) for _ in range(2)]
        rec[f"fused_{tag}_flags"] = [bool(eng._delta_step), bool(eng._knot_step), bool(eng._whole_step)]
        # ... announcing the next batch, then on the workspace that batch was binned into
        ws2 = torch.empty_like(eng.ws)
        idx, nidx = torch.arange(B), torch.arange(B, 2 * B)
        rec[f"fused_{tag}_next"] = names(lambda: eng._enqueue(None, coords, t, y, B, B, idx=idx, nxt=(nidx, ws2)))
        rec[f"fused_{tag}_prebinned"] = names(lambda: eng._enqueue(None, coords, t, y, B, B, idx=nidx, ws=ws2,
                                                                   prebinned=True, nxt=(idx, eng.ws)))
        rec[f"fused_{tag}_prebinned_last"] = names(lambda: eng._enqueue(None, None, None, y, B, B, ws=ws2, prebinned=True))
        eng = _engine(_model(DENSE, False, learn, True), fused_delta_step=True)
        rec[f"fused_{tag}_dense"] = one(eng)
        eng = _engine(_model(WIN, True, learn, True))
        rec[f"default_{tag}"] = [one(eng) for _ in range(2)]
        rec[f"default_{tag}_flags"] = [bool(eng._delta_step), bool(eng._knot_step), bool(eng._whole_step)]
        # the environment switch: quietly, only where the path applies
        os.environ["STNF_FUSED_DELTA_STEP"] = "1"
        try:
            eng = _engine(_model(WIN, True, learn, True))
            rec[f"env_{tag}"] = one(eng)
            eng = _engine(_model(WIN, True, learn, False))                   # no delta head: today's path
            rec[f"env_{tag}_no_head"] = one(eng)
            eng = _engine(_model(WIN, True, learn, True), world_size=2)       # virtual rank of two: the split calls
            rec[f"env_{tag}_world2_flag"] = bool(eng._delta_step)
            eng = _engine(_model(WIN, True, learn, True), fused_delta_step=False)
            rec[f"env_{tag}_false_flag"] = bool(eng._delta_step)
        finally:
            del os.environ["STNF_FUSED_DELTA_STEP"]
        # the config key through make_engine
        cfg = dict(regression_type="multi-quantile", quantile_levels=TAUS5, use_delta_reparameterization=True,
                   non_crossing_lambda=1.0, grad_clip=10.0, fused_delta_step=True)
        eng = T.make_engine(_model(WIN, True, learn, True), cfg, B, 4)
        rec[f"config_{tag}"] = one(eng)
        eng = T.make_engine(_model(WIN, True, learn, True), dict(cfg, fused_delta_step=False), B, 4)
        rec[f"config_{tag}_off"] = one(eng)

    # ValueErrors of fused_delta_step=True / fused_knot_step=True
    def refusal(make):
        try:
            make()
        except (ValueError, RuntimeError) as e:
            return f"{type(e).__name__}: {e}"
        return None

    class _FakeStream:
        cuda_stream = 0x1000

    rec["raise_no_head"] = refusal(lambda: _engine(_model(WIN, True, False, False), fused_delta_step=True))
    rec["raise_world"] = refusal(lambda: _engine(_model(WIN, True, False, True), fused_delta_step=True, world_size=2))
    torch.cuda.Stream = lambda device=None: _FakeStream()        # (no device here: two_streams only needs a handle)
    rec["raise_two_streams"] = refusal(lambda: _engine(_model(WIN, True, False, True), fused_delta_step=True,
                                                       two_streams=True))
    rec["raise_knot_step_on_delta"] = refusal(lambda: _engine(_model(WIN, True, True, True), fused_knot_step=True))
    eng = _engine(_model(WIN, True, True, True), fused_knot_step=True, fused_delta_step=True)
    rec["both_true_flags"] = [bool(eng._delta_step), bool(eng._knot_step)]

    # ---- what the door refuses, each with its text; the descriptors are a fused engine's own
    N.lib = lambda: real

    def door_errors(learn):
        eng = _engine(_model(WIN, True, learn, True), fused_delta_step=True)
        eng.step(None, coords[:B], t[:B], y[:B])
        st = eng.state
        plan = eng._cached("one_call", eng._plan_key(), eng._one_call_plan)
        L, Q = st.desc.n_hidden, 5
        head = lambda: N.make_delta_step(st.delta, eng.d_delta, 1.0, float(B * Q))

        def call(head_=None, desc=None, grads=None, flags=None, knots="own", d_centers="own", no_head=False):
            h = None if no_head else (head_ if head_ is not None else head())
            kn = (eng._knot_train_desc(B * Q), eng.g_centers, eng.g_log_bw, plan[1]) if learn else (None,) * 4
            if knots != "own":
                kn = kn[:3] + (knots,)
            if d_centers != "own":
                kn = (kn[0], d_centers) + kn[2:]
            return refusal(lambda: N.train_step_delta(
                st.basis, desc or st.desc, st.params, grads or eng.grads_t, coords[:B], t[:B], None, y[:B], None, B,
                1.0 / (B * Q), eng.loss_sum, eng.ws, st.flags if flags is None else flags, plan[0], h, *kn, None, seed=7,
                loss_desc=eng.objective.desc(1)))

        out = {"ok": call()}
        out["null_head"] = call(no_head=True)
        d1 = N.MlpDesc.from_buffer_copy(st.desc)
        d1.out_dim = 1
        out["q_below_2"] = call(desc=d1)
        h = head(); h.ldd = h.ldg = 3
        out["ldd_small"] = call(h)
        h = head(); h.ldg = h.ldd + 4
        out["strides_differ"] = call(h)
        apart = lambda like: torch.zeros(like.shape[0], like.stride(0))[:, :like.shape[1]]     # same shape and stride
        out["delta_outside"] = call(N.make_delta_step(apart(st.delta), eng.d_delta, 1.0, 1.0))
        out["d_delta_outside"] = call(N.make_delta_step(st.delta, apart(eng.d_delta), 1.0, 1.0))
        g2 = N.MlpTensors.from_buffer_copy(eng.grads_t)
        g2.W[L] = eng.grad[eng.knot_end:].data_ptr()
        out["scratch_inside"] = call(grads=g2)
        if learn:
            out["pack_with_knots"] = call(flags=st.flags | N.FLAG_PACK_F32)
            kg = N.AdamGroup.from_buffer_copy(plan[1])
            table = N.BF16Shadow()
            kg.shadow = C.pointer(table)
            out["knot_shadow"] = call(knots=kg)
            out["mixture_no_d_centers"] = call(d_centers=None)
        else:
            out["mixture_d_centers_only"] = call(d_centers=torch.zeros(4, 2))
        return out

    rec["door_fixed"] = door_errors(False)
    rec["door_learn"] = door_errors(True)
    return rec


_cache = {}


def _recorded():
    if "rec" not in _cache:
        env = dict(os.environ, STDADK_DRY_RUN="1")
        for k in ENV_SWITCHES:
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        line = [l for l in r.stdout.splitlines() if l.startswith("RECORD ")][-1]
        _cache["rec"] = json.loads(line[len("RECORD "):])
    return _cache["rec"]


# ------------------------------------------------------------------------------------------------ tests: calls
@pytest.mark.parametrize("tag", ["fixed", "learn"])
def test_a_fused_step_is_one_call(tag):
    rec = _recorded()["calls"]
    assert rec[f"fused_{tag}_flags"] == [True, False, False]
    for one in rec[f"fused_{tag}"] + [rec[f"fused_{tag}_dense"], rec[f"env_{tag}"], rec[f"config_{tag}"]]:
        assert one["calls"] == [DOOR], one
    # a next batch announced on the window route at 64 rows: carried (True), then the step on the pre-binned workspace
    assert rec[f"fused_{tag}_next"] == {"calls": [DOOR], "ret": True}
    assert rec[f"fused_{tag}_prebinned"] == {"calls": [DOOR], "ret": True}
    assert rec[f"fused_{tag}_prebinned_last"]["calls"] == [DOOR]
    assert "delta_head_f32" not in rec[f"fused_{tag}"][0]["calls"]


@pytest.mark.parametrize("tag,split", [("fixed", SPLIT_FIXED), ("learn", SPLIT_LEARN)])
def test_default_engines_make_todays_calls(tag, split):
    rec = _recorded()["calls"]
    assert rec[f"default_{tag}_flags"] == [False, False, False]
    for one in rec[f"default_{tag}"] + [rec[f"config_{tag}_off"]]:
        assert one["calls"] == split, one
    # the switch is quiet where the path does not apply, and False wins over it
    assert DOOR not in rec[f"env_{tag}_no_head"]["calls"] and rec[f"env_{tag}_no_head"]["calls"]
    assert rec[f"env_{tag}_world2_flag"] is False and rec[f"env_{tag}_false_flag"] is False


def test_value_errors_name_their_reason():
    rec = _recorded()["calls"]
    assert rec["raise_no_head"].startswith("ValueError: fused_delta_step=True needs a model with the delta head")
    assert rec["raise_world"].startswith("ValueError: fused_delta_step=True needs a single process")
    assert rec["raise_two_streams"].startswith("ValueError: fused_delta_step=True needs two_streams=False")
    # unchanged (tests/test_knot_step_cpu.py pins it too): the knots door alone still refuses a delta model
    assert rec["raise_knot_step_on_delta"] == ("ValueError: fused_knot_step=True needs a model without the delta head "
                                               "(use_delta_reparameterization=False)")
    assert rec["both_true_flags"] == [True, False]


REFUSALS = {
    "null_head": "train_step_delta: head is NULL",
    "q_below_2": "train_step_delta: Q=1 outside 2..8",
    "ldd_small": "train_step_delta: ldd=3 below d + 1 = 65",
    "strides_differ": "train_step_delta: the strides of delta (",
    "delta_outside": "train_step_delta: delta [Q,ldd] lies outside the parameter range",
    "d_delta_outside": "train_step_delta: d_delta [Q,ldd] lies outside the gradient range",
    "scratch_inside": "train_step_delta: grads->W[L] / b[L] (scratch of the derived output layer) lie inside the gradient",
    "pack_with_knots": "train_step_delta: flags carry STDADK_FLAG_PACK_F32",
    "knot_shadow": "train_step_delta: knots->shadow must be NULL",
    "mixture_no_d_centers": "train_step_delta: kt / d_centers / d_log_bw / knots given in part",
    "mixture_d_centers_only": "train_step_delta: kt / d_centers / d_log_bw / knots given in part",
}


@pytest.mark.parametrize("tag", ["fixed", "learn"])
def test_every_refusal_of_the_door_comes_with_its_text(tag):
    rec = _recorded()["calls"][f"door_{tag}"]
    assert rec.pop("ok") is None                         # the same call, unaltered, is accepted
    only = {"fixed": {"mixture_d_centers_only"}, "learn": {"pack_with_knots", "knot_shadow", "mixture_no_d_centers"}}
    want = (set(REFUSALS) - only["fixed"] - only["learn"]) | only[tag]
    assert set(rec) == want, (sorted(rec), sorted(want))
    for k, msg in rec.items():
        assert msg is not None and "stdadk_train_step_delta_f32 failed (code -1)" in msg and REFUSALS[k] in msg, (k, msg)


# ------------------------------------------------------------------------------------------------ tests: chains
def test_every_chain_is_recorded():
    assert sorted(_recorded()["chains"]) == sorted(expected_chains())
    assert set(GPU_CASES) <= set(expected_chains())


@pytest.mark.parametrize("name", sorted(expected_chains()) if os.path.exists(FIXTURE) else [])
def test_launch_chain(name):
    got, want = _recorded()["chains"][name], expected_chains()[name]
    assert want and got == want, (name, got, want)


def _pair(case):
    e = expected_chains()
    return e[f"delta/{case}"], e[f"twin/{case}"]


@pytest.mark.parametrize("case", ["learn_window", "learn_dense", "learn_window_noclip"])
def test_learnable_chain_is_the_twins_with_the_head_in_front(case):
    delta, twin = _pair(case)
    assert delta == ["delta_head_kernel"] + twin, (delta, twin)
    assert delta.count("step_finish_kernel") == 1


@pytest.mark.parametrize("case,added", [("fixed_window", 0), ("fixed_window_dw_fin1", 0), ("fixed_dense", 0),
                                        ("fixed_window_noclip", 0), ("fixed_window_dw_fin2", 1),
                                        ("fixed_window_dw_fin0", 1)])
def test_fixed_chain_has_the_finishing_launch_where_the_twin_reduces(case, added):
    """The twin's chain with delta_head_kernel in front and step_finish_kernel where the twin has its reductions launch;
    one launch more where the twin has none (finishing mode 2).  Mode 0 (diagnostic) also has one more: its 256 region
    workgroups stay a reductions launch of their own in front of the finishing launch, as in learnable steps."""
    delta, twin = _pair(case)
    twin = [k for k in twin if k != "step_advance_kernel"]       # (clipping off: the finishing launch carries the advance)
    assert delta[0] == "delta_head_kernel" and len(delta) == len(twin) + 1 + added, (delta, twin)
    if added == 0:
        assert delta[1:] == [("step_finish_kernel" if k == "reduce_jobs_kernel" else k) for k in twin], (delta, twin)
        assert "reduce_jobs_kernel" in twin
    elif case.endswith("fin2"):
        assert "reduce_jobs_kernel" not in twin
        assert delta[1:] == twin[:-1] + ["step_finish_kernel"] + twin[-1:], (delta, twin)
    else:
        assert delta[1:] == twin[:-1] + ["step_finish_kernel"] + twin[-1:], (delta, twin)
    assert delta.count("step_finish_kernel") == 1 and delta[-1] == twin[-1]


@pytest.mark.parametrize("case", sorted(c[len("delta/"):] for c in (expected_chains() if os.path.exists(FIXTURE) else [])
                                        if c.startswith("delta/")))
def test_no_sumsq_launch_where_the_twin_has_none(case):
    delta, twin = _pair(case)
    has = lambda chain: any("sumsq" in k for k in chain)
    assert has(delta) == has(twin), (delta, twin)
    assert not any(k.startswith("delta_head_bwd") for k in delta)
    if "sparsity" in case:            # the norm is a pass of its own, behind the finishing launch
        assert has(delta) and delta.index("step_finish_kernel") < [i for i, k in enumerate(delta) if "sumsq" in k][0]


if __name__ == "__main__":
    print("RECORD " + json.dumps({"calls": _record_calls(), "chains": record_chains()}, sort_keys=True))
    sys.exit(0)
