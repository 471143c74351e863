"""Call-trace guard of stnf.engine.TrainStep (CPU, no GPU): which library entry points one optimisation step calls, in
which order and with which arguments, for every kind of step the engine enqueues.  A change of the host code that moves
a launch, an argument or a buffer offset shows here before anything runs on a device.

How: with STDADK_DRY_RUN=1 every entry point of libstdadk validates and plans but launches nothing, and TrainStep runs
on host tensors.  This file is its own driver: started as a script in a child process (stnf._native reads the variable at
import) it wraps the object returned by `_native.lib()` in a proxy and writes, for every call made during a step, the
entry point, every scalar argument (floats as the float32 the ABI takes) and, for every pointer -- arguments and the
fields of the descriptors alike -- the NAME of the engine buffer the address falls in plus the offset in elements (the
lengths are the scalar arguments / `n` fields next to them), so the record does not depend on where the allocator put
things.  AdamGroup / OptimDesc / BF16Shadow descriptors are written out in full; the model-level descriptors (basis,
MLP, parameter and gradient tables, loss, sparsity, knot penalties) as a digest of the same normalised form
(`--verbose` writes them out too).  The stream argument is not recorded.

`python tests/test_engine_call_trace.py [--engine path/to/another/engine.py] [--verbose]` prints the record as JSON;
with --engine the TrainStep of that file is driven instead (comparing two versions of the host code)."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 64


# ------------------------------------------------------------------------------------------------ the driver
def _record(engine_path=None, verbose=False):
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    import torch
    from stnf import _native as N
    from stnf.models import STInterpMLP
    if engine_path:
        spec = importlib.util.spec_from_file_location("stnf.engine", engine_path)
        E = importlib.util.module_from_spec(spec)
        sys.modules["stnf.engine"] = E
        spec.loader.exec_module(E)
    else:
        from stnf import engine as E

    real = N.lib()
    state = {"eng": None, "extra": {}, "log": [], "built": 0}
    FULL = (N.AdamGroup, N.OptimDesc, N.BF16Shadow, N.BF16Region)

    def buffers():
        eng = state["eng"]
        out = []
        # (a view comes after the buffer it is a view of: the sharded engine's `sumsq` lies in `_sumsq_all`)
        for name in ("flat", "grad", "m", "v", "ema", "ws", "_sumsq_all", "sumsq", "sumsq_basis", "_sumsq512", "lr_dev",
                     "basis_lr_dev", "step_dev", "loss_sum", "nonfinite", "_shadow_buf", "_pack_buf"):
            tns = getattr(eng, name, None)
            if tns is not None:
                out.append((name.replace("_shadow_buf", "bf16_shadow").replace("_pack_buf", "pack"), tns))
        for i, tns in enumerate(eng.d_head or []):
            out += [(f"head{i}", eng.state.head[i]), (f"d_head{i}", tns)]
        for name, tns in eng.model.named_buffers():
            out.append((f"buffer:{name}", tns))
        ev = state.get("ev")
        if ev is not None:
            # the evaluator's accumulator, workspaces (by flags) and, in bf16 mode, its operand copies of the EMA values
            out.append(("eval_acc", ev.acc))
            out += [(f"eval_ws{flags}", tns) for flags, tns in sorted(ev._ws.items())]
            if ev._ema is not None:
                for l, pair in enumerate(ev._ema[1]._views[1] or []):
                    if pair is not None:
                        out += [(f"eval_bf16_w{l}", pair[0]), (f"eval_bf16_wt{l}", pair[1])]
        return out + list(state["extra"].items())

    def where(addr):
        if not addr:
            return "null"
        for name, tns in buffers():
            base = tns.data_ptr()
            if tns.numel() and base <= addr < base + tns.numel() * tns.element_size():
                return f"{name}+{(addr - base) // tns.element_size()}"
        return "other"

    def value(ctype, v):
        """Normalised form of one argument / field of C type `ctype`."""
        if isinstance(ctype, type) and issubclass(ctype, C.Array):
            return [value(ctype._type_, x) for x in v]
        if isinstance(ctype, type) and issubclass(ctype, C.Structure):
            return struct(v)
        if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
            if v is None or (isinstance(v, C._Pointer) and not v):
                return "null"
            obj = v._obj if hasattr(v, "_obj") else v.contents          # byref(x) | pointer(x)
            if not isinstance(obj, C.Structure):
                return "out"                                            # (int32 *prepared of train_step_next)
            return struct(obj)
        if ctype is C.c_void_p:
            return where(v.value if isinstance(v, C.c_void_p) else v)
        if ctype is C.c_float:
            return float(f"{C.c_float(v).value:.9g}")
        if ctype is C.c_double:
            return float(v)                             # (the batch weight of eval_indexed)
        return int(v)

    def struct(obj):
        d = {name: value(ctype, getattr(obj, name)) for name, ctype in obj._fields_}
        if isinstance(obj, N.BF16Shadow):
            d["r"] = d["r"][:d["n"]]
        if isinstance(obj, N.MlpTensors):
            d = {k: [x for x in v if x != "null"] for k, v in d.items()}
        if isinstance(obj, FULL) or verbose:
            return "{" + " ".join(f"{k}={v}" for k, v in d.items()).replace("'", "") + "}"
        return type(obj).__name__ + ":" + hashlib.sha1(json.dumps(d, sort_keys=True).encode()).hexdigest()[:10]

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name in ("stdadk_last_error", "stdadk_abi_version"):
                return fn

            def call(*args):
                types = N._SIGNATURES[name][1]
                if state["eng"] is None:            # (an engine under construction: planning calls, not a step)
                    return fn(*args)
                state["log"].append([name.replace("stdadk_", "")] + [value(t, a) for t, a in zip(types[:-1], args)])
                return fn(*args)
            return call

    proxy = Proxy()
    N.lib = lambda: proxy
    make_group = N.make_adam_group

    def counting_make_group(*a, **kw):
        state["built"] += 1
        return make_group(*a, **kw)
    N.make_adam_group = counting_make_group

    def model(hidden_dims=(64, 64), **kw):
        torch.manual_seed(0)
        return STInterpMLP(p=0, k_spatial_centers=[25, 81], k_temporal_centers=[10, 15], hidden_dims=list(hidden_dims),
                           dropout=0.1, layernorm=True, **kw).train()

    g = torch.Generator().manual_seed(1)
    data = (torch.rand(B, 2, generator=g), torch.rand(B, 1, generator=g), torch.randn(B, 1, generator=g))

    def engine(model_kw, eng_kw):
        state["eng"] = state["ev"] = None
        eng = E.TrainStep(model(**model_kw), max_batch=B, ema_decay=0.99, seed=7, **eng_kw)
        c, t, y = data
        state["eng"], state["extra"] = eng, {"coords": c, "t": t, "y": y}
        return eng, c, t, y

    def take():
        out = {"calls": state["log"], "groups_built": state["built"]}
        state["log"], state["built"] = [], 0
        return out

    def run(model_kw, eng_kw, between=None, steps=3):
        eng, c, t, y = engine(model_kw, eng_kw)
        take()
        out = []
        for i in range(steps):
            if between is not None:
                between(eng, i)
            eng.step(None, c, t, y)
            out.append(take())
        return out

    def run_sharded(model_kw, eng_kw, steps=3):
        """Two virtual ranks of the sharded optimiser driven by hand, as tests/test_gpu_round3.py does (the collectives
        are the caller's in this mode)."""
        eng, c, t, y = engine(model_kw, dict(eng_kw, world_size=2, shard_optimizer=True))
        take()
        out = []
        for _ in range(steps):
            for r in range(2):
                eng.set_virtual_rank(r)
                eng._enqueue_grads(None, c, t.view(-1), y, B, 2 * B)
                eng._shard_sumsq()
                eng._shard_adamw()
                out.append(dict(take(), rank=r, lo=eng.lo, hi=eng.hi, knot_end=eng.knot_end))
            eng._stepped(2 * B)
        return out

    def run_by_hand(model_kw, eng_kw, steps=3):
        """The split halves driven by hand on a single-GPU engine, as tools and the virtual-rank tests drive them: on an
        engine that streams packed fp32 copies the split optimiser launch must not be handed those (it would round bf16
        into them; only the one-call launch writes fragment order)."""
        eng, c, t, y = engine(model_kw, eng_kw)
        take()
        out = []
        for _ in range(steps):
            eng._enqueue_grads(None, c, t.view(-1), y, B, B)
            eng._shard_sumsq()
            eng._shard_adamw()
            out.append(take())
            eng._stepped(B)
        return out

    def run_eval(eng_kw, params, passes=3):
        """Evaluator.evaluate over a 150-row host set at batch_size = 64: two full batches and a ragged one.  Every pass
        is recorded like a step (nothing may change from pass to pass)."""
        from stnf.dataio.device_dataset import DeviceDataset
        from stnf.evaluation import Evaluator
        eng, _, _, _ = engine({}, eng_kw)
        g2 = torch.Generator().manual_seed(2)
        ds = DeviceDataset(torch.rand(150, 2, generator=g2), torch.rand(150, 1, generator=g2),
                           torch.randn(150, 1, generator=g2))
        batches = ds.epoch_batches

        def named_batches(*a, **kw):            # the index slices are views of one tensor made per pass: name it
            out = batches(*a, **kw)
            state["extra"]["idx"] = out[0]._base if out[0]._base is not None else out[0]
            return out
        ds.epoch_batches = named_batches
        state["ev"] = ev = Evaluator(eng.model, max_batch=B)
        state["extra"] = {"ds_coords": ds.coords, "ds_t": ds.t, "ds_y": ds.y}
        take()
        out = []
        for _ in range(passes):
            ev.evaluate(ds, B, params=params, engine=eng)
            out.append(take())
        return out

    def rates(eng, i):
        if i == 1:
            eng.set_lr(1e-2)
        if i == 2:
            eng.set_basis_lr(5e-4)

    def lr_only(eng, i):
        if i == 1:
            eng.set_lr(1e-2)

    learn = {"spatial_learnable": True}
    taus = [0.05, 0.25, 0.5, 0.75, 0.95]
    rec = {
        "knot_one_call": run(learn, {"fused_knot_step": True}),
        "knot_one_call_noclip": run(learn, {"fused_knot_step": True, "grad_clip": 0}),
        "knot_one_call_rates": run(learn, {"fused_knot_step": True}, between=rates, steps=4),
        "whole_rates": run({}, {}, between=lr_only),                   # set_lr before step 2
        "whole_packed": run({"hidden_dims": (128, 128)}, {}),
        "packed_split_by_hand": run_by_hand({"hidden_dims": (128, 128)}, {}),
        "whole_sparsity": run({}, {"sparsity_penalty_type": "sparse_group"}),
        "whole_pinball": run({"output_dim": 5}, {"loss": "pinball", "quantile_levels": taus,
                                                 "non_crossing_weight": 0.1}),
        "eval_live": run_eval({}, "live"),
        "eval_ema": run_eval({}, "ema"),
        "eval_ema_bf16": run_eval({"dtype": "bf16"}, "ema"),
        "whole": run({}, {}),
        "whole_noclip": run({}, {"grad_clip": 0}),
        "split": run({}, {"world_size": 2}),
        "split_noclip": run({}, {"world_size": 2, "grad_clip": 0}),
        "split_bf16": run({}, {"world_size": 2, "dtype": "bf16"}),
        "split_sparsity": run({}, {"world_size": 2, "sparsity_penalty_type": "sparse_group"}),
        "delta_head": run({"output_dim": 5, "use_delta_reparameterization": True},
                          {"loss": "pinball", "quantile_levels": taus, "non_crossing_lambda": 0.05}),
        "learnable": run(learn, {}),
        "learnable_noclip": run(learn, {"grad_clip": 0}),
        "learnable_bf16": run(learn, {"dtype": "bf16"}),
        "learnable_rates": run(learn, {}, between=rates, steps=4),     # set_lr before step 2, set_basis_lr before 3
        "sharded": run_sharded({}, {}),
        "sharded_noclip": run_sharded({}, {"grad_clip": 0}),
        "sharded_learnable": run_sharded(learn, {}),
        "sharded_learnable_noclip": run_sharded(learn, {"grad_clip": 0}),
        "sharded_learnable_bf16": run_sharded(learn, {"dtype": "bf16"}),
    }
    return rec


def record_in_child(engine_path=None):
    env = dict(os.environ, STDADK_DRY_RUN="1")
    cmd = [sys.executable, os.path.abspath(__file__)] + (["--engine", engine_path] if engine_path else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout)


# ------------------------------------------------------------------------------------------------ the pinned record
# Calls of the FIRST step of every configuration (model: [25, 81] knots, [10, 15] temporal centres, hidden [64, 64],
# B = 64, ema_decay = 0.99, seed = 7), one list per virtual rank for the sharded ones.  Later steps repeat them with the
# host's step number advanced (_at_step): nothing else may change from step to step -- a cache that goes stale or a
# descriptor built from the wrong step would show.  Written by `python tests/test_engine_call_trace.py` and compared
# with the record of the engine before the optimiser paths were merged into one plan (--engine): equal, except that
# 'learnable_noclip' launched adamw_ema_f32 twice (MLP group, then knot group) where it now launches adamw_ema2_f32
# once, as the sharded engine always has for that configuration.
EXPECTED = {'whole': [[['train_step_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
             'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 'null', 64, 0.015625, 'null', 'null',
             'loss_sum+0', 'ws+0', 215040, 7, 2,
             '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=12932 lr=0.0199999996 lr_dev=lr_dev+0 beta1=0.899999976 '
             'beta2=0.999000013 eps=9.99999994e-09 weight_decay=0.000500000024 step_dev=step_dev+0 max_norm=10.0 '
             'sumsq_parts=_sumsq512+0 ema_decay=0.99000001 shadow=null nonfinite_step=nonfinite+0}']]],
 'whole_noclip': [[['train_step_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
                    'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 'null', 64, 0.015625, 'null', 'null',
                    'loss_sum+0', 'ws+0', 215040, 7, 2,
                    '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=12932 lr=0.0199999996 lr_dev=lr_dev+0 '
                    'beta1=0.899999976 beta2=0.999000013 eps=9.99999994e-09 weight_decay=0.000500000024 '
                    'step_dev=step_dev+0 max_norm=0.0 sumsq_parts=null ema_decay=0.99000001 shadow=null '
                    'nonfinite_step=nonfinite+0}']]],
 'split': [[['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
             'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null', 'loss_sum+0', 'null',
             'ws+0', 215040, 7, 'step_dev+0', 2, 'null'],
            ['sumsq_f32', 'grad+0', 12932, 'sumsq+0', 'step_dev+0'],
            ['adamw_ema_f32', 'flat+0', 'grad+0', 'm+0', 'v+0', 'ema+0', 12932, 0.0199999996, 'lr_dev+0',
             0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 10.0, 'sumsq+0', 256, 1.0,
             0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']]],
 'split_noclip': [[['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
                    'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null', 'loss_sum+0',
                    'null', 'ws+0', 215040, 7, 'step_dev+0', 2, 'null'],
                   ['step_advance', 'step_dev+0'],
                   ['adamw_ema_f32', 'flat+0', 'grad+0', 'm+0', 'v+0', 'ema+0', 12932, 0.0199999996, 'lr_dev+0',
                    0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 0.0, 'sumsq+0', 256,
                    1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']]],
 'split_bf16': [[['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:d53ed29842',
                  'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null', 'loss_sum+0',
                  'null', 'ws+0', 215040, 7, 'step_dev+0', 34, 'null'],
                 ['sumsq_f32', 'grad+0', 12932, 'sumsq+0', 'step_dev+0'],
                 ['adamw_ema_f32', 'flat+0', 'grad+0', 'm+0', 'v+0', 'ema+0', 12932, 0.0199999996, 'lr_dev+0',
                  0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 10.0, 'sumsq+0', 256,
                  1.0, 0.99000001, '{n=1 r=[{off=8576 rows=64 cols=64 dst=bf16_shadow+0 dst_t=bf16_shadow+4096}]}',
                  'loss_sum+0', 'nonfinite+0']]],
 'split_sparsity': [[['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
                      'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null',
                      'loss_sum+0', 'null', 'ws+0', 215040, 7, 'step_dev+0', 2, 'null'],
                     ['sparsity_f32', 'SparsityDesc:cba14e6b23', 'flat+0', 'grad+0', 64, 1, 64, 0, 106, 25, 0.5,
                      64.0, 'loss_sum+0', 'null'],
                     ['sumsq_f32', 'grad+0', 12932, 'sumsq+0', 'step_dev+0'],
                     ['adamw_ema_f32', 'flat+0', 'grad+0', 'm+0', 'v+0', 'ema+0', 12932, 0.0199999996, 'lr_dev+0',
                      0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 10.0, 'sumsq+0',
                      256, 1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']]],
 'delta_head': [[['delta_head_f32', 'flat+12864', 68, 5, 64, 'head0+0', 'head1+0'],
                 ['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:da7468e423', 'MlpTensors:51708485aa',
                  'MlpTensors:9163538900', 'coords+0', 't+0', 'null', 'y+0', 64, 0.00312500005,
                  'LossDesc:60d1c5a25d', 'loss_sum+0', 'null', 'ws+0', 219392, 7, 'step_dev+0', 2, 'null'],
                 ['delta_head_backward_f32', 'flat+12864', 'd_head0+0', 'd_head1+0', 68, 5, 64, 0.0500000007, 16.0,
                  'grad+12864', 'loss_sum+0'],
                 ['sumsq_f32', 'grad+0', 13204, 'sumsq+0', 'step_dev+0'],
                 ['adamw_ema_f32', 'flat+0', 'grad+0', 'm+0', 'v+0', 'ema+0', 13204, 0.0199999996, 'lr_dev+0',
                  0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 10.0, 'sumsq+0', 256,
                  1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']]],
 'learnable': [[['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
                 'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0', 64, 0.015625, 'null', 'loss_sum+0',
                 'null', 'ws+0', 217344, 7, 'step_dev+0', 6, 'null'],
                ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
                 'coords+0', 64, 'ws+0', 217344, 6, 'KnotTrain:20b933dfe6', 'grad+0', 'grad+212', 'loss_sum+0'],
                ['sumsq2_f32', 'grad+320', 12932, 'sumsq+0', 'grad+0', 320, 'sumsq_basis+0', 'step_dev+0'],
                ['adamw_ema2_f32',
                 '{p=flat+320 g=grad+320 m=m+320 v=v+320 ema=ema+320 n=12932 lr=0.0199999996 lr_dev=lr_dev+0 '
                 'max_norm=10.0 sumsq_parts=sumsq+0 n_parts=256 shadow=null}',
                 '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=320 lr=0.00100000005 lr_dev=basis_lr_dev+0 '
                 'max_norm=1.0 sumsq_parts=sumsq_basis+0 n_parts=256 shadow=null}',
                 0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 1.0, 0.99000001,
                 'loss_sum+0', 'nonfinite+0']]],
 'learnable_noclip': [[['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
                        'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0', 64, 0.015625, 'null',
                        'loss_sum+0', 'null', 'ws+0', 217344, 7, 'step_dev+0', 6, 'null'],
                       ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
                        'coords+0', 64, 'ws+0', 217344, 6, 'KnotTrain:20b933dfe6', 'grad+0', 'grad+212',
                        'loss_sum+0'],
                       ['step_advance', 'step_dev+0'],
                       ['adamw_ema2_f32',
                        '{p=flat+320 g=grad+320 m=m+320 v=v+320 ema=ema+320 n=12932 lr=0.0199999996 '
                        'lr_dev=lr_dev+0 max_norm=0.0 sumsq_parts=sumsq+0 n_parts=256 shadow=null}',
                        '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=320 lr=0.00100000005 lr_dev=basis_lr_dev+0 '
                        'max_norm=0.0 sumsq_parts=sumsq_basis+0 n_parts=256 shadow=null}',
                        0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 1.0, 0.99000001,
                        'loss_sum+0', 'nonfinite+0']]],
 'learnable_bf16': [[['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:a33f39e740',
                      'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0', 64, 0.015625, 'null', 'loss_sum+0',
                      'null', 'ws+0', 217344, 7, 'step_dev+0', 38, 'null'],
                     ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:a33f39e740',
                      'coords+0', 64, 'ws+0', 217344, 38, 'KnotTrain:20b933dfe6', 'grad+0', 'grad+212',
                      'loss_sum+0'],
                     ['sumsq2_f32', 'grad+320', 12932, 'sumsq+0', 'grad+0', 320, 'sumsq_basis+0', 'step_dev+0'],
                     ['adamw_ema2_f32',
                      '{p=flat+320 g=grad+320 m=m+320 v=v+320 ema=ema+320 n=12932 lr=0.0199999996 lr_dev=lr_dev+0 '
                      'max_norm=10.0 sumsq_parts=sumsq+0 n_parts=256 shadow={n=1 r=[{off=8576 rows=64 cols=64 '
                      'dst=bf16_shadow+0 dst_t=bf16_shadow+4096}]}}',
                      '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=320 lr=0.00100000005 lr_dev=basis_lr_dev+0 '
                      'max_norm=1.0 sumsq_parts=sumsq_basis+0 n_parts=256 shadow=null}',
                      0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 1.0, 0.99000001,
                      'loss_sum+0', 'nonfinite+0']]],
 'sharded': [[['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
               'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null', 'loss_sum+0',
               'null', 'ws+0', 215040, 7, 'step_dev+0', 2, 'null'],
              ['sumsq_f32', 'grad+0', 6496, '_sumsq_all+0', 'step_dev+0'],
              ['adamw_ema_f32', 'flat+0', 'grad+0', 'm+0', 'v+0', 'ema+0', 6496, 0.0199999996, 'lr_dev+0',
               0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 10.0, '_sumsq_all+0', 256,
               1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']],
             [['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
               'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null', 'loss_sum+0',
               'null', 'ws+0', 215040, 15111065706836454666, 'step_dev+0', 2, 'null'],
              ['sumsq_f32', 'grad+6496', 6496, '_sumsq_all+0', 'step_dev+0'],
              ['adamw_ema_f32', 'flat+6496', 'grad+6496', 'm+0', 'v+0', 'ema+0', 6496, 0.0199999996, 'lr_dev+0',
               0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 10.0, '_sumsq_all+0', 256,
               1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']]],
 'sharded_noclip': [[['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
                      'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null',
                      'loss_sum+0', 'null', 'ws+0', 215040, 7, 'step_dev+0', 2, 'null'],
                     ['step_advance', 'step_dev+0'],
                     ['adamw_ema_f32', 'flat+0', 'grad+0', 'm+0', 'v+0', 'ema+0', 6496, 0.0199999996, 'lr_dev+0',
                      0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 0.0,
                      '_sumsq_all+0', 256, 1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']],
                    [['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:d72abd2a12', 'MlpTensors:4152523d56',
                      'MlpTensors:35fb96d573', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null',
                      'loss_sum+0', 'null', 'ws+0', 215040, 15111065706836454666, 'step_dev+0', 2, 'null'],
                     ['step_advance', 'step_dev+0'],
                     ['adamw_ema_f32', 'flat+6496', 'grad+6496', 'm+0', 'v+0', 'ema+0', 6496, 0.0199999996,
                      'lr_dev+0', 0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 0.0,
                      '_sumsq_all+0', 256, 1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']]],
 'sharded_learnable': [[['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
                         'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null',
                         'loss_sum+0', 'null', 'ws+0', 217344, 7, 'step_dev+0', 6, 'null'],
                        ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
                         'coords+0', 64, 'ws+0', 217344, 6, 'KnotTrain:9283a3a330', 'grad+0', 'grad+212',
                         'loss_sum+0'],
                        ['sumsq2_f32', 'grad+320', 6336, '_sumsq_all+0', 'grad+0', 320, '_sumsq_all+256',
                         'step_dev+0'],
                        ['adamw_ema2_f32',
                         '{p=flat+320 g=grad+320 m=m+320 v=v+320 ema=ema+320 n=6336 lr=0.0199999996 '
                         'lr_dev=lr_dev+0 max_norm=10.0 sumsq_parts=_sumsq_all+0 n_parts=256 shadow=null}',
                         '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=320 lr=0.00100000005 lr_dev=basis_lr_dev+0 '
                         'max_norm=1.0 sumsq_parts=_sumsq_all+256 n_parts=256 shadow=null}',
                         0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 1.0, 0.99000001,
                         'loss_sum+0', 'nonfinite+0']],
                       [['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
                         'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0', 64, 0.0078125, 'null',
                         'loss_sum+0', 'null', 'ws+0', 217344, 15111065706836454666, 'step_dev+0', 6, 'null'],
                        ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
                         'coords+0', 64, 'ws+0', 217344, 6, 'KnotTrain:9283a3a330', 'grad+0', 'grad+212',
                         'loss_sum+0'],
                        ['sumsq2_f32', 'grad+6656', 6656, '_sumsq_all+0', 'null', 0, '_sumsq_all+256',
                         'step_dev+0'],
                        ['adamw_ema_f32', 'flat+6656', 'grad+6656', 'm+0', 'v+0', 'ema+0', 6656, 0.0199999996,
                         'lr_dev+0', 0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0',
                         10.0, '_sumsq_all+0', 256, 1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']]],
 'sharded_learnable_noclip': [[['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12',
                                'MlpTensors:dddfd30ce4', 'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0',
                                64, 0.0078125, 'null', 'loss_sum+0', 'null', 'ws+0', 217344, 7, 'step_dev+0', 6,
                                'null'],
                               ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12',
                                'MlpTensors:dddfd30ce4', 'coords+0', 64, 'ws+0', 217344, 6, 'KnotTrain:9283a3a330',
                                'grad+0', 'grad+212', 'loss_sum+0'],
                               ['step_advance', 'step_dev+0'],
                               ['adamw_ema2_f32',
                                '{p=flat+320 g=grad+320 m=m+320 v=v+320 ema=ema+320 n=6336 lr=0.0199999996 '
                                'lr_dev=lr_dev+0 max_norm=0.0 sumsq_parts=null n_parts=0 shadow=null}',
                                '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=320 lr=0.00100000005 '
                                'lr_dev=basis_lr_dev+0 max_norm=0.0 sumsq_parts=null n_parts=0 shadow=null}',
                                0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 1.0,
                                0.99000001, 'loss_sum+0', 'nonfinite+0']],
                              [['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12',
                                'MlpTensors:dddfd30ce4', 'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0',
                                64, 0.0078125, 'null', 'loss_sum+0', 'null', 'ws+0', 217344, 15111065706836454666,
                                'step_dev+0', 6, 'null'],
                               ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12',
                                'MlpTensors:dddfd30ce4', 'coords+0', 64, 'ws+0', 217344, 6, 'KnotTrain:9283a3a330',
                                'grad+0', 'grad+212', 'loss_sum+0'],
                               ['step_advance', 'step_dev+0'],
                               ['adamw_ema_f32', 'flat+6656', 'grad+6656', 'm+0', 'v+0', 'ema+0', 6656,
                                0.0199999996, 'lr_dev+0', 0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024,
                                1, 'step_dev+0', 0.0, '_sumsq_all+0', 256, 1.0, 0.99000001, 'null', 'loss_sum+0',
                                'nonfinite+0']]],
 'sharded_learnable_bf16': [[['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12',
                              'MlpTensors:a33f39e740', 'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0',
                              64, 0.0078125, 'null', 'loss_sum+0', 'null', 'ws+0', 217344, 7, 'step_dev+0', 38,
                              'null'],
                             ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12',
                              'MlpTensors:a33f39e740', 'coords+0', 64, 'ws+0', 217344, 38, 'KnotTrain:9283a3a330',
                              'grad+0', 'grad+212', 'loss_sum+0'],
                             ['sumsq2_f32', 'grad+320', 6336, '_sumsq_all+0', 'grad+0', 320, '_sumsq_all+256',
                              'step_dev+0'],
                             ['adamw_ema2_f32',
                              '{p=flat+320 g=grad+320 m=m+320 v=v+320 ema=ema+320 n=6336 lr=0.0199999996 '
                              'lr_dev=lr_dev+0 max_norm=10.0 sumsq_parts=_sumsq_all+0 n_parts=256 shadow=null}',
                              '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=320 lr=0.00100000005 '
                              'lr_dev=basis_lr_dev+0 max_norm=1.0 sumsq_parts=_sumsq_all+256 n_parts=256 '
                              'shadow=null}',
                              0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 1.0,
                              0.99000001, 'loss_sum+0', 'nonfinite+0']],
                            [['train_fwd_bwd_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12',
                              'MlpTensors:a33f39e740', 'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0',
                              64, 0.0078125, 'null', 'loss_sum+0', 'null', 'ws+0', 217344, 15111065706836454666,
                              'step_dev+0', 38, 'null'],
                             ['knot_backward_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12',
                              'MlpTensors:a33f39e740', 'coords+0', 64, 'ws+0', 217344, 38, 'KnotTrain:9283a3a330',
                              'grad+0', 'grad+212', 'loss_sum+0'],
                             ['sumsq2_f32', 'grad+6656', 6656, '_sumsq_all+0', 'null', 0, '_sumsq_all+256',
                              'step_dev+0'],
                             ['adamw_ema_f32', 'flat+6656', 'grad+6656', 'm+0', 'v+0', 'ema+0', 6656, 0.0199999996,
                              'lr_dev+0', 0.899999976, 0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0',
                              10.0, '_sumsq_all+0', 256, 1.0, 0.99000001, 'null', 'loss_sum+0', 'nonfinite+0']]]}


# What landed on the engine after that record -- the one-call learnable step, the packed fp32 weights, the one-call step
# with a sparsity penalty / the pinball objective, the validation pass -- recorded with the host layer as it was before
# its bookkeeping was put on one flat layout, one optimiser plan and one step call, and equal to what that layer
# produces now.  One difference, in 'whole_rates' (test_one_call_descriptor_follows_set_lr): the one-call step's
# descriptor used to be built once without a key, so its host-side `lr` field kept the constructor's rate after set_lr;
# it now comes from the keyed plan and carries the new rate.  No kernel reads that field when `lr_dev` is given
# (optim.hip: a.lr_dev ? a.lr_dev[0] : a.lr), and the engine always gives it.
_ONE_CALL_OPTIM = ('{p=flat+%d g=grad+%d m=m+%d v=v+%d ema=ema+%d n=%d lr=0.0199999996 lr_dev=lr_dev+0 '
                   'beta1=0.899999976 beta2=0.999000013 eps=9.99999994e-09 weight_decay=0.000500000024 '
                   'step_dev=step_dev+0 max_norm=%s sumsq_parts=%s ema_decay=0.99000001 shadow=%s '
                   'nonfinite_step=nonfinite+0}')


def _knot_one_call(max_norm, parts, knot_norm, knot_parts, n_parts):
    return [[['train_step_knots_f32', 'BasisDesc:00f7db00d5', 'MlpDesc:d72abd2a12', 'MlpTensors:dddfd30ce4',
              'MlpTensors:b19767907e', 'coords+0', 't+0', 'null', 'y+0', 'null', 64, 0.015625, 'null', 'null',
              'loss_sum+0', 'ws+0', 217344, 7, 6,
              _ONE_CALL_OPTIM % (320, 320, 320, 320, 320, 12932, max_norm, parts, 'null'),
              'null', 0, 0, 'null', 0, 'out', 'KnotTrain:20b933dfe6', 'grad+0', 'grad+212',
              '{p=flat+0 g=grad+0 m=m+0 v=v+0 ema=ema+0 n=320 lr=0.00100000005 lr_dev=basis_lr_dev+0 '
              f'max_norm={knot_norm} sumsq_parts={knot_parts} n_parts={n_parts} shadow=null}}']]]


def _whole(mlp, tensors, grads, scale, loss, sparsity, ws_bytes, flags, n, shadow='null'):
    return [[['train_step_f32', 'BasisDesc:a6984a6617', mlp, tensors, grads, 'coords+0', 't+0', 'null', 'y+0', 'null',
              64, scale, loss, sparsity, 'loss_sum+0', 'ws+0', ws_bytes, 7, flags,
              _ONE_CALL_OPTIM % (0, 0, 0, 0, 0, n, '10.0', '_sumsq512+0', shadow)]]]


def _eval_pass(tensors, flags, first=()):
    """150 rows at batch_size = 64: the workspace query, then two full batches and the ragged one."""
    return [list(first) + [['eval_workspace_bytes', 'BasisDesc:a6984a6617', 'MlpDesc:a487f0a014', 64]] + [
        ['eval_indexed_f32', 'BasisDesc:a6984a6617', 'MlpDesc:a487f0a014', tensors, 'ds_coords+0', 'ds_t+0', 'null',
         'ds_y+0', f'idx+{o}', n, 'null', 0, 1.0 / n, 'eval_acc+0', 'null', f'eval_ws{flags}+0', 306432, flags]
        for o, n in ((0, 64), (64, 64), (128, 22))]]


EXPECTED.update({
    'knot_one_call': _knot_one_call('10.0', '_sumsq512+0', '1.0', 'sumsq_basis+0', 256),
    'knot_one_call_noclip': _knot_one_call('0.0', 'null', '0.0', 'null', 0),
    'whole_packed': _whole('MlpDesc:90c3542bfa', 'MlpTensors:c441924c5d', 'MlpTensors:2340bbcb42', 0.015625, 'null',
                           'null', 388096, 130, 34052,
                           '{n=1 r=[{off=17152 rows=128 cols=128 dst=pack+0 dst_t=pack+16384}]}'),
    # the split halves by hand on that engine: the weights themselves, and NO table of copies in the optimiser launch
    'packed_split_by_hand': [[
        ['train_fwd_bwd_f32', 'BasisDesc:a6984a6617', 'MlpDesc:90c3542bfa', 'MlpTensors:29b31c311a',
         'MlpTensors:2340bbcb42', 'coords+0', 't+0', 'null', 'y+0', 64, 0.015625, 'null', 'loss_sum+0', 'null', 'ws+0',
         388096, 7, 'step_dev+0', 2, 'null'],
        ['sumsq_f32', 'grad+0', 34052, 'sumsq+0', 'step_dev+0'],
        ['adamw_ema_f32', 'flat+0', 'grad+0', 'm+0', 'v+0', 'ema+0', 34052, 0.0199999996, 'lr_dev+0', 0.899999976,
         0.999000013, 9.99999994e-09, 0.000500000024, 1, 'step_dev+0', 10.0, 'sumsq+0', 256, 1.0, 0.99000001, 'null',
         'loss_sum+0', 'nonfinite+0']]],
    'whole_sparsity': _whole('MlpDesc:d72abd2a12', 'MlpTensors:4152523d56', 'MlpTensors:35fb96d573', 0.015625, 'null',
                             'SparsityDesc:cba14e6b23', 215040, 2, 12932),
    'whole_pinball': _whole('MlpDesc:da7468e423', 'MlpTensors:9625a35ad0', 'MlpTensors:8ba923e048', 0.00312500005,
                            'LossDesc:0cb00ecdb3', 'null', 219392, 2, 13192),
    'eval_live': _eval_pass('MlpTensors:4152523d56', 2),
    'eval_ema': _eval_pass('MlpTensors:27ccbc4963', 2),
    'eval_ema_bf16': _eval_pass('MlpTensors:293fbf428c', 34, first=[
        ['bf16_shadow_refresh', 'ema+0',
         '{n=1 r=[{off=8576 rows=64 cols=64 dst=eval_bf16_w1+0 dst_t=eval_bf16_wt1+0}]}']]),
})
assert EXPECTED['whole_sparsity'][0][0][-1] == EXPECTED['whole'][0][0][-1]      # (the descriptor the first record pins)

RATES = {"learnable_rates", "knot_one_call_rates", "whole_rates"}     # pinned by tests of their own, below
STEP_ARG = {"adamw_ema_f32": 13, "adamw_ema2_f32": 7}       # position of the host step number in a recorded call
# descriptors built per step: the plan of the non-sharded engines is built in the first step and never again; the
# one-call step has its own descriptor; an engine that plays two virtual ranks in turn holds ONE plan and rebuilds it at
# every switch (set_virtual_rank moves lo / hi and the moment buffers, which are in the plan's key)
GROUPS_BUILT = {"whole": [0, 0, 0], "whole_noclip": [0, 0, 0], "split": [1, 0, 0], "split_noclip": [1, 0, 0],
                "split_bf16": [1, 0, 0], "split_sparsity": [1, 0, 0], "delta_head": [1, 0, 0], "learnable": [2, 0, 0],
                "learnable_noclip": [2, 0, 0], "learnable_bf16": [2, 0, 0], "learnable_rates": [2, 2, 2, 0],
                "sharded": [1, 1] * 3, "sharded_noclip": [1, 1] * 3, "sharded_learnable": [2, 1] * 3,
                "sharded_learnable_noclip": [2, 1] * 3, "sharded_learnable_bf16": [2, 1] * 3,
                # the one-call learnable step builds one group descriptor (the knots'; the MLP's is an OptimDesc); the
                # validation pass builds none
                "knot_one_call": [1, 0, 0], "knot_one_call_noclip": [1, 0, 0], "knot_one_call_rates": [1, 1, 1, 0],
                "whole_rates": [0, 0, 0], "whole_packed": [0, 0, 0], "packed_split_by_hand": [1, 0, 0],
                "whole_sparsity": [0, 0, 0],
                "whole_pinball": [0, 0, 0], "eval_live": [0, 0, 0], "eval_ema": [0, 0, 0], "eval_ema_bf16": [0, 0, 0]}
SLICES = {False: [(0, 6496, 0), (6496, 12992, 0)], True: [(0, 6656, 320), (6656, 13312, 320)]}    # (lo, hi, knot_end)
_cache = {}


def _at_step(calls, k, subs=()):
    out = []
    for c in calls:
        c = list(c)
        if c[0] in STEP_ARG:
            c[STEP_ARG[c[0]]] = k
        for old, new in subs:
            c = [a.replace(old, new) if isinstance(a, str) else a for a in c]
        out.append(c)
    return out


def _recorded():
    if "rec" not in _cache:
        _cache["rec"] = record_in_child()
    return _cache["rec"]


def test_every_configuration_is_recorded():
    assert set(_recorded()) == set(EXPECTED) | RATES == set(GROUPS_BUILT)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_library_calls_of_three_consecutive_steps(name):
    steps = _recorded()[name]
    ranks = len(EXPECTED[name])
    assert len(steps) == 3 * ranks
    for i, got in enumerate(steps):
        assert got["calls"] == _at_step(EXPECTED[name][i % ranks], i // ranks + 1), (name, i)
        if ranks == 2:
            assert (got["lo"], got["hi"], got["knot_end"]) == SLICES["learnable" in name][got["rank"]]
    assert [s["groups_built"] for s in steps] == GROUPS_BUILT[name]


def test_plan_is_rebuilt_exactly_when_a_rate_changes():
    """set_lr before step 2, set_basis_lr before step 3, nothing before step 4: the group descriptors carry the new
    rate from the step after the change on, and are rebuilt in exactly those steps."""
    _rates_follow("learnable_rates", "learnable", 3)


def test_one_call_learnable_plan_is_rebuilt_exactly_when_a_rate_changes():
    _rates_follow("knot_one_call_rates", "knot_one_call", 0)


def _rates_follow(name, base, call):
    steps = _recorded()[name]
    first = EXPECTED[base][0]
    lr, basis = ("lr=0.0199999996", "lr=0.00999999978"), ("lr=0.00100000005", "lr=0.000500000024")
    assert sum(a.count(lr[0]) + a.count(basis[0]) for a in first[call] if isinstance(a, str)) == 2
    for k, subs in enumerate([(), (lr,), (lr, basis), (lr, basis)], start=1):
        assert steps[k - 1]["calls"] == _at_step(first, k, subs), k
    assert [s["groups_built"] for s in steps] == GROUPS_BUILT[name]


def test_one_call_descriptor_follows_set_lr():
    """set_lr before step 2 of the one-call step: the descriptor's host-side rate follows (the kernels read lr_dev)."""
    steps = _recorded()["whole_rates"]
    first = EXPECTED["whole"][0]
    lr = ("lr=0.0199999996", "lr=0.00999999978")
    assert first[0][-1].count(lr[0]) == 1
    for k, subs in enumerate([(), (lr,), (lr,)], start=1):
        assert steps[k - 1]["calls"] == _at_step(first, k, subs), k
    assert [s["groups_built"] for s in steps] == GROUPS_BUILT["whole_rates"]


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--engine") + 1] if "--engine" in sys.argv else None
    json.dump(_record(path, "--verbose" in sys.argv), sys.stdout)
    sys.exit(0)
