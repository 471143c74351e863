"""The one-call learnable-knot step (stdadk_train_step_knots_f32, TrainStep(fused_knot_step=...)) on the host: which
library calls a step makes, when the engine takes the path, and what the door refuses (CPU, no GPU).

How (as tests/test_engine_call_trace.py): with STDADK_DRY_RUN=1 every entry point of libstdadk validates and plans but
launches nothing, and TrainStep runs on host tensors.  This file is its own driver: started as a script in a child
process (stnf._native reads the variable at import) it records the names of the entry points called per step and the
error text of every refused call, and prints them as JSON."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 64
DOOR = "train_step_knots_f32"
SPLIT = ["train_fwd_bwd_f32", "knot_backward_f32", "sumsq2_f32", "adamw_ema2_f32"]


# ------------------------------------------------------------------------------------------------ the driver
def _record():
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    import torch
    from stnf import _native as N
    from stnf import training as T
    from stnf.engine import TrainStep
    from stnf.models import STInterpMLP

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

    def model(window=False, **kw):
        torch.manual_seed(0)
        kw.setdefault("spatial_learnable", True)
        m = STInterpMLP(p=0, k_spatial_centers=[25, 81], k_temporal_centers=[10, 15],
                        hidden_dims=[128, 64] if window else [64, 64], dropout=0.1, layernorm=True, **kw).train()
        if window:
            m.force_window_path = True
        return m

    g = torch.Generator().manual_seed(1)
    n = 4 * B
    coords, t, y = torch.rand(n, 2, generator=g), torch.rand(n, generator=g), torch.randn(n, 1, generator=g)

    def names(fn):
        del log[:]
        out = fn()
        return {"calls": list(log), "ret": out}

    def engine(m=None, **kw):
        return TrainStep(m if m is not None else model(), max_batch=B, ema_decay=0.99, seed=7, **kw)

    rec = {}
    # --- which calls a learnable step makes
    eng = engine(fused_knot_step=True)
    rec["fused"] = [names(lambda: eng.step(None, coords[:B], t[:B], y[:B])) for _ in range(2)]
    rec["fused_flags"] = [bool(eng._knot_step), bool(eng._whole_step)]
    eng = engine()
    rec["default"] = [names(lambda: eng.step(None, coords[:B], t[:B], y[:B])) for _ in range(2)]
    rec["default_flags"] = [bool(eng._knot_step), bool(eng._whole_step)]
    os.environ["STNF_FUSED_KNOT_STEP"] = "1"
    try:
        eng = engine()
        rec["env"] = [names(lambda: eng.step(None, coords[:B], t[:B], y[:B]))]
        rec["env_flags"] = [bool(eng._knot_step), bool(eng._whole_step)]
        quiet = engine(model(spatial_learnable=False))            # None: quietly the path that applies
        rec["env_fixed_flags"] = [bool(quiet._knot_step), bool(quiet._whole_step)]
        os.environ["STNF_FUSED_KNOT_STEP"] = "0"
        rec["env_off_flags"] = [bool(engine()._knot_step)]
    finally:
        del os.environ["STNF_FUSED_KNOT_STEP"]
    # window path, rows `idx` of the resident arrays, the NEXT batch announced: what _step_pipelined enqueues
    eng = engine(model(window=True), fused_knot_step=True)
    assert eng.uses_window
    perm = torch.randperm(n, generator=g)
    ws2 = torch.empty_like(eng.ws)
    rec["next"] = [names(lambda: eng._enqueue(None, coords, t, y, B, B, idx=perm[:B], nxt=(perm[B:2 * B], ws2))),
                   names(lambda: eng._enqueue(None, coords, t, y, B, B, idx=perm[B:2 * B], ws=ws2, prebinned=True,
                                              nxt=(perm[2 * B:3 * B], eng.ws))),
                   names(lambda: eng._enqueue(None, coords, t, y, B, B, idx=perm[:B]))]

    # --- where fused_knot_step=True does not apply
    def raised(fn):
        try:
            fn()
        except ValueError as e:
            return str(e)
        return None
    taus = [0.05, 0.25, 0.5, 0.75, 0.95]
    rec["value_errors"] = {
        "world": raised(lambda: engine(fused_knot_step=True, world_size=2)),
        "delta": raised(lambda: engine(model(output_dim=5, use_delta_reparameterization=True), fused_knot_step=True,
                                       loss="pinball", quantile_levels=taus, non_crossing_lambda=0.05)),
        "fixed": raised(lambda: engine(model(spatial_learnable=False), fused_knot_step=True)),
    }

    # --- make_engine passes the config key
    cfg = {"lr": 1e-3, "batch_size": B, "grad_clip": 10.0}
    rec["make_engine"] = [bool(T.make_engine(model(), dict(cfg, fused_knot_step=True), B, 4)._knot_step),
                          bool(T.make_engine(model(), cfg, B, 4)._knot_step)]

    # --- what the door refuses
    eng = engine(fused_knot_step=True)
    st = eng.state
    optim, knots = eng._knot_step_plan()
    kt = eng._knot_train_desc(B)

    def door(flags=None, d_centers=None, knots_=None, kt_=None):
        try:
            N.train_step_knots(st.basis, st.desc, st.params, eng.grads_t, coords[:B], t[:B], None, y[:B], None, B, 1.0 / B,
                               eng.loss_sum, eng.ws, st.flags if flags is None else flags, optim,
                               kt if kt_ is None else kt_, eng.g_centers if d_centers is None else d_centers,
                               eng.g_log_bw, knots if knots_ is None else knots_, seed=7)
        except RuntimeError as e:
            return str(e)
        return None

    def group(**kw):
        gr = N.AdamGroup.from_buffer_copy(knots)
        for k, v in kw.items():
            setattr(gr, k, v)
        return gr
    shadow = N.make_bf16_shadow([(0, 16, 16, torch.empty(256, dtype=torch.bfloat16), None)])
    sb = eng.model.spatial_basis
    no_init = N.make_knot_train(None, True, sb.damping_threshold, sb.damping_strength)
    rec["refused"] = {
        "accepted": door(),
        "log_bw": door(flags=st.flags & ~N.FLAG_LOG_BW),
        "pack_f32": door(flags=st.flags | N.FLAG_PACK_F32),
        "d_centers": door(d_centers=eng.grad[eng.knot_end:eng.knot_end + 2 * sb.k].view(sb.k, 2)),
        "shadow": door(knots_=group(shadow=C.pointer(shadow))),
        "partials": door(knots_=group(sumsq_parts=None, max_norm=1.0)),
        "centers_init": door(kt_=no_init),
    }
    rec["after_refusals"] = names(lambda: eng.step(None, coords[:B], t[:B], y[:B]))["calls"]
    return rec


_cache = {}


def _recorded():
    if "rec" not in _cache:
        env = dict(os.environ, STDADK_DRY_RUN="1")
        env.pop("STNF_FUSED_KNOT_STEP", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        _cache["rec"] = json.loads(r.stdout)
    return _cache["rec"]


# ------------------------------------------------------------------------------------------------ the tests
def test_fused_learnable_step_is_one_library_call():
    rec = _recorded()
    assert rec["fused_flags"] == [True, False]           # (_whole_step keeps its meaning: one parameter group)
    for s in rec["fused"]:
        assert s["calls"] == [DOOR], s
        assert s["ret"] is None


def test_default_learnable_step_keeps_the_four_calls():
    rec = _recorded()
    assert rec["default_flags"] == [False, False]
    for s in rec["default"]:
        assert s["calls"] == SPLIT, s


def test_environment_variable_turns_the_path_on():
    rec = _recorded()
    assert rec["env_flags"] == [True, False]
    assert rec["env"][0]["calls"] == [DOOR]
    assert rec["env_fixed_flags"] == [False, True]       # None: a fixed-knot engine quietly stays what it was
    assert rec["env_off_flags"] == [False]               # anything but "1" leaves it off


def test_one_call_with_and_without_an_announced_next_batch():
    """Window path on rows `idx` of the resident arrays, as _step_pipelined enqueues it: the door alone, whether the
    next batch is announced or not and whether this one arrives binned or not; the library reports the announced
    batch as binned (the weight-gradient launch carries it)."""
    first, second, last = _recorded()["next"]
    assert first["calls"] == second["calls"] == last["calls"] == [DOOR]
    assert first["ret"] is True and second["ret"] is True and last["ret"] is False


@pytest.mark.parametrize("case,word", [("world", "world size"), ("delta", "delta head"), ("fixed", "learnable knots")])
def test_explicit_request_where_the_path_does_not_apply_raises(case, word):
    msg = _recorded()["value_errors"][case]
    assert msg is not None and "fused_knot_step=True" in msg and word in msg, msg


def test_make_engine_passes_the_config_key():
    assert _recorded()["make_engine"] == [True, False]


@pytest.mark.parametrize("case,argument", [("log_bw", "STDADK_FLAG_LOG_BW"), ("pack_f32", "STDADK_FLAG_PACK_F32"),
                                           ("d_centers", "d_centers"), ("shadow", "knots->shadow"),
                                           ("partials", "knots->sumsq_parts"), ("centers_init", "centers_init")])
def test_the_door_refuses(case, argument):
    rec = _recorded()["refused"]
    assert rec["accepted"] is None, rec["accepted"]          # the same call with nothing wrong goes through
    msg = rec[case]
    assert msg is not None, case
    assert "stdadk_train_step_knots_f32 failed (code -1)" in msg and "train_step_knots" in msg and argument in msg, msg
    assert _recorded()["after_refusals"] == [DOOR]


def test_symbol_is_declared_and_exported():
    from stnf import _native as N
    hdr = open(os.path.join(ROOT, "include", "stdadk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+stdadk_train_step_knots_f32\s*\(", hdr)
    assert "stdadk_train_step_knots_f32" in N.exported_symbols()
    assert hasattr(C.CDLL(N.LIB_PATH), "stdadk_train_step_knots_f32")
    assert int(re.search(r"#define\s+STDADK_ABI_VERSION\s+(\d+)", hdr).group(1)) == N.ABI_VERSION == 10


if __name__ == "__main__":
    json.dump(_record(), sys.stdout)
    sys.exit(0)
