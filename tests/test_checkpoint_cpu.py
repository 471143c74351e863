"""CPU tests of TrainStep.state_dict / load_state_dict, stnf.checkpoint and train_model(checkpoint=, resume=) (no GPU):
with STDADK_DRY_RUN=1 the library validates and plans but launches nothing, so what is saved, what a load writes and
refuses, and the driver's control flow across a cut can be checked on host tensors.  stnf._native reads the variable at
import, so this file is its own driver (the pattern of test_training_cpu.py): run as a script in a child process it
prints one JSON record, which the tests read."""
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, EPOCHS, BATCH, ROWS, VAL_ROWS = 2e-2, 8, 64, 200, 150
LOSSES = [0.9, 0.5, float("nan"), 0.7, 0.4, 0.45, 0.41, 0.6]
CUTS = list(range(1, 8))
SCHED = ["sched_fixed", "sched_learn", "sched_learn_now"]


class Killed(Exception):
    """The process 'dies' here: raised by a scripted evaluator in place of a time limit."""


def _record(tmp):
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    import torch
    from stnf import _native as N
    from stnf import checkpoint as CK
    from stnf import engine as E
    from stnf import training as T
    from stnf.dataio.device_dataset import DeviceDataset
    from stnf.engine import TrainStep
    from stnf.models import STInterpMLP

    def model(seed=0, hidden=(64, 64), **kw):
        torch.manual_seed(seed)
        return STInterpMLP(p=0, k_spatial_centers=[25, 81], k_temporal_centers=[10, 15], hidden_dims=list(hidden),
                           dropout=0.0, layernorm=True, **kw)

    def data(n, seed):
        g = torch.Generator().manual_seed(seed)
        return DeviceDataset(torch.rand(n, 2, generator=g), torch.rand(n, 1, generator=g), torch.randn(n, 1, generator=g))

    class Stub:
        """Scripted validation losses; dies (Killed) when the script runs out.  A dry run never changes the shadow, so
        the stub stamps it: after the validation of epoch e (1-based, `first` epochs were run before this process)
        every element of `engine.ema` is e -- a best state, a model or a model_best.pt says which epoch it is from."""
        def __init__(self, losses, first=0):
            self.losses, self.calls, self.first = list(losses), 0, first

        def evaluate(self, dataset, batch_size, params="live", engine=None):
            self.calls += 1
            if self.calls > len(self.losses):
                raise Killed()
            if engine is not None and engine.ema is not None:
                with torch.no_grad():
                    engine.ema.fill_(float(self.first + self.calls))
            v = self.losses[self.calls - 1]
            return {"loss": v, "rmse": abs(v) ** 0.5 if v == v else v, "mse": v, "mae": v}

    rec = {}
    tr, va = data(ROWS, 1), data(VAL_ROWS, 2)

    # --- 1. round trip through a file into an engine of another initialisation and another dropout seed
    def tensors_of(eng):
        out = {"flat": eng.flat, "m": eng.m, "v": eng.v, "ema": eng.ema, "step_dev": eng.step_dev,
               "loss_sum": eng.loss_sum, "nonfinite": eng.nonfinite, "lr_dev": eng.lr_dev}
        if eng.learnable:
            out["basis_lr_dev"] = eng.basis_lr_dev
        out.update({"buffers." + n: b for n, b in eng.model.named_buffers()})
        return out

    def scribble(eng, seed):
        """Dry-run steps change no buffer: put recognisable values into everything a step would have written."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, t in tensors_of(eng).items():
                if name in ("lr_dev", "basis_lr_dev"):
                    continue
                if t.dtype == torch.int32:
                    t.fill_(seed)
                else:
                    t.copy_(torch.randn(t.shape, generator=g))

    def round_trip(name, world=None, **kw):
        a = TrainStep(model(0, **kw), lr=LR, grad_clip=10.0, ema_decay=0.99, max_batch=BATCH, seed=5, world_size=world,
                      domain_penalty_weight=0.01 if kw else 0.0)
        idx = torch.arange(BATCH)
        for _ in range(3):
            a.step_indexed(tr.coords, tr.t, tr.y, idx)
        scribble(a, 7)
        a.set_lr(0.003)
        if a.learnable:
            a.set_basis_lr(0.0004)
        path = os.path.join(tmp, name + ".pt")
        rng = torch.get_rng_state()
        CK.save_checkpoint(path, a, extra={"note": name})
        rng_kept = bool(torch.equal(rng, torch.get_rng_state()))
        b = TrainStep(model(1, **kw), lr=LR, grad_clip=10.0, ema_decay=0.99, max_batch=BATCH, seed=9, world_size=world,
                      domain_penalty_weight=0.01 if kw else 0.0)
        if world:
            b.set_virtual_rank(1)
        different = not torch.equal(a.flat, b.flat)
        before = {k: t.data_ptr() for k, t in tensors_of(b).items()}
        b._prepared = E._Announced((1, 2, 3), 0, idx, True)            # an announced batch and two captured chains
        b._graph.key, b._graph.graph = "k", object()
        b._ix_graph.key, b._ix_graph.graph = "k", object()
        version = getattr(b.model, "_engine_version", 0)
        extra = CK.load_checkpoint(path, b)
        ta, tb = tensors_of(a), tensors_of(b)
        return {"different_before": different, "rng_kept": rng_kept, "extra": extra,
                "equal": {k: bool(torch.equal(ta[k], tb[k])) for k in ta},
                "same_address": {k: tb[k].data_ptr() == before[k] for k in tb},
                "prepared_none": b._prepared is None,
                "graphs_stale": [b._graph.stale("k"), b._ix_graph.stale("k")],
                "version_bumped": getattr(b.model, "_engine_version", 0) > version,
                "seed": [b.seed, E._rank_seed(5, b.rank), b.base_seed, b.rank],
                "counters": [b.step_count, b.rows_seen, a.step_count, a.rows_seen],
                "rates": [b.lr, float(b.lr_dev[0]), a.lr] + ([b.basis_lr, float(b.basis_lr_dev[0]), a.basis_lr]
                                                             if b.learnable else [])}
    rec["round_trip"] = {"fixed": round_trip("fixed"), "learn": round_trip("learn", spatial_learnable=True),
                         "rank1": round_trip("rank1", world=2)}

    # --- 2. refusals
    def refusal(saver, loader):
        try:
            loader.load_state_dict(saver if isinstance(saver, dict) else saver.state_dict())
            return ["ok", ""]
        except (ValueError, NotImplementedError) as e:
            return [type(e).__name__, str(e)]

    def eng(seed=0, hidden=(64, 64), **kw):
        a = dict(lr=LR, grad_clip=10.0, ema_decay=0.99, max_batch=BATCH, seed=5)
        a.update(kw)
        return TrainStep(model(seed, hidden), **a)
    base = eng()
    bad_format = base.state_dict()
    bad_format["format"] = 99
    shard = eng(world_size=2, shard_optimizer=True)

    def raises_not_implemented(fn):
        try:
            fn()
            return ["ok", ""]
        except NotImplementedError as e:
            return ["NotImplementedError", str(e)]
    def in_swap_pair(fn):
        """RuntimeError between the two swap_in_ema calls of a pair (the buffers are exchanged), fine after it."""
        e = eng()
        out = []
        for _ in range(2):
            e.swap_in_ema()
            try:
                fn(e)
                out.append("ok")
            except RuntimeError as err:
                out.append("RuntimeError: " + str(err))
        return out
    flat_before = base.flat.clone()
    rec["refusals"] = {"same": refusal(base, eng(1)), "hidden": refusal(base, eng(hidden=(64, 32))),
                       "dtype": refusal(base, eng(dtype="bf16")), "dtype_back": refusal(eng(dtype="bf16"), base),
                       "ema_missing": refusal(base, eng(ema_decay=None)),
                       "ema_extra": refusal(eng(ema_decay=None), base),
                       "grad_clip": refusal(base, eng(grad_clip=5.0)), "format": refusal(bad_format, eng()),
                       "weight_decay": refusal(base, eng(weight_decay=1e-3)),
                       "world": refusal(base, eng(world_size=2)),
                       "shard_save": raises_not_implemented(shard.state_dict),
                       "shard_load": raises_not_implemented(lambda: shard.load_state_dict(base.state_dict())),
                       "swap_save": in_swap_pair(lambda e: e.state_dict()),
                       "swap_load": in_swap_pair(lambda e: e.load_state_dict(base.state_dict())),
                       "step_call": refusal(*(TrainStep(model(0, spatial_learnable=True), lr=LR, grad_clip=10.0,
                                                        ema_decay=0.99, max_batch=BATCH, seed=5, fused_knot_step=fused)
                                              for fused in (True, False))),
                       "untouched": bool(torch.equal(flat_before, base.flat))}

    # --- 3. the file: plain data, and a write that dies leaves the previous checkpoint alone
    path = os.path.join(tmp, "file.pt")
    base.step_count = 11
    CK.save_checkpoint(path, base, extra={"n": 1})
    plain = torch.load(path, map_location="cpu", weights_only=True)
    base.step_count = 12
    save = torch.save

    def dying_save(obj, f, *a, **kw):
        save(obj, f, *a, **kw)
        raise OSError("killed after writing")
    torch.save = dying_save
    try:
        CK.save_checkpoint(path, base, extra={"n": 2})
        died = False
    except OSError:
        died = True
    finally:
        torch.save = save
    again = eng(1)
    extra = CK.load_checkpoint(path, again)
    rec["file"] = {"keys": sorted(plain), "engine_format": plain["engine"]["format"], "died": died, "extra": extra,
                   "step_count": again.step_count}

    # --- 4. the reference's schedules across a cut after every epoch
    from golden import training_cases as tc
    rec["sched"] = {}
    for name in SCHED:
        case = tc.SCHED_CASES[name]
        c = dict(case["config"], verbose=False)
        nb = math.ceil(tc.SCHED_ROWS / tc.SCHED_BATCH)
        losses = [1.0 / (i + 1) for i in range(c["epochs"])]
        rec["sched"][name] = {}
        for cut in CUTS:
            path = os.path.join(tmp, f"{name}_{cut}.pt")
            per_step, lr_col = [], None
            for leg, script in enumerate((losses[:cut], losses[cut:])):
                m = model(leg, spatial_learnable=True) if case["learnable"] else model(leg)
                e = T.make_engine(m, c, tc.SCHED_BATCH, nb)
                step, mine = e.step_indexed, []

                def stepping(*a, _step=step, _e=e, _out=mine, _learn=case["learnable"], **kw):
                    _out.append([_e.lr, float(_e.lr_dev[0])] + ([_e.basis_lr, float(_e.basis_lr_dev[0])] if _learn else []))
                    return _step(*a, **kw)
                e.step_indexed = stepping
                try:
                    _, hist, _ = T.train_model(m, data(tc.SCHED_ROWS, 1), data(tc.SCHED_VAL_ROWS, 2), c, shuffle=False,
                                               engine=e, evaluator=Stub(script), checkpoint=path, resume=leg == 1)
                    lr_col = hist["lr"]
                except Killed:
                    mine = mine[:cut * nb]         # the epoch it died in is repeated by the resumed run
                per_step += mine
            rec["sched"][name][str(cut)] = {"rates": per_step, "lr": lr_col}

    # --- 5. best state, patience and early stop across the cut; resuming the finished run
    cfg = {"lr": LR, "epochs": EPOCHS, "batch_size": BATCH, "warmup_epochs": 1, "scheduler": "cosine", "patience": 3,
           "grad_clip": 10.0, "verbose": False}
    n_batches = math.ceil(ROWS / BATCH)

    def values(tensors):
        """The distinct values in `tensors` (the stub's stamps: one value = one epoch) and a checksum of them all."""
        flat = torch.cat([t.detach().double().reshape(-1) for t in tensors])
        return {"distinct": sorted(set(flat.tolist()))[:4], "sum": float(flat.sum()), "numel": flat.numel()}

    def run(tag, script, seed=0, first=0, epochs=EPOCHS, **kw):
        c = dict(cfg, epochs=epochs)
        m = model(seed)
        e = T.make_engine(m, c, BATCH, n_batches)
        out_dir = os.path.join(tmp, tag)
        stub = Stub(script, first)
        try:
            _, hist, _ = T.train_model(m, tr, va, c, output_dir=out_dir, shuffle=False, engine=e, evaluator=stub, **kw)
        except Killed:
            return None
        sd = torch.load(os.path.join(out_dir, "model_best.pt"))
        return {"hist": hist, "files": sorted(os.listdir(out_dir)), "steps": e.step_count, "stub_calls": stub.calls,
                "csv": open(os.path.join(out_dir, "training_history.csv")).read().splitlines(),
                "keys": sorted(sd), "best_is_model": all(torch.equal(sd[k], v) for k, v in m.state_dict().items()),
                # (the file also holds the model's buffers, the knot tables: the parameters are what the stamp marks)
                "best_file": values([sd[k] for k, _ in m.named_parameters()]), "best_ema": values([e.best_ema]),
                "model": values(list(m.parameters())), "shadow": values([e.ema]),
                "val_script_left": len(stub.losses) - stub.calls}

    def saved_driver_state(path):
        x = torch.load(path, map_location="cpu", weights_only=True)["extra"]
        return {"epoch": x["epoch"], "stopped": x["stopped"], "best_val": x["best_val"],
                "patience_counter": x["patience_counter"], "has_best": x["has_best"],
                "best_state": values([x["best_state"]]) if x["best_state"] is not None else None}
    # epochs = 8: the issue's case (patience runs out in the last epoch); epochs = 10: only the restored patience
    # counter and best value can stop the resumed run after the 8th epoch -- epochs 9 and 10 would both be best
    rec["patience"] = {}
    for epochs, script in ((EPOCHS, LOSSES), (10, LOSSES + [0.3, 0.2])):
        r = rec["patience"][str(epochs)] = {"whole": run(f"whole_{epochs}", script, epochs=epochs)}
        for cut in (5, 6):
            path = os.path.join(tmp, f"patience_{epochs}_{cut}.pt")
            assert run(f"dies_{epochs}_{cut}", script[:cut], epochs=epochs, checkpoint=path) is None
            r[f"{cut}_saved"] = saved_driver_state(path)
            r[str(cut)] = run(f"resumed_{epochs}_{cut}", script[cut:], seed=1, first=cut, epochs=epochs, checkpoint=path,
                              resume=True)
            r[f"{cut}_again"] = run(f"again_{epochs}_{cut}", [], seed=2, first=8, epochs=epochs, checkpoint=path,
                                    resume=True)
    # resume=True without a file is a run from epoch 0; checkpoint_every=3 still saves the last epoch
    path = os.path.join(tmp, "every3.pt")
    rec["patience"]["no_file"] = run("no_file", LOSSES, checkpoint=path, checkpoint_every=3, resume=True)
    last = torch.load(path, map_location="cpu", weights_only=True)["extra"]
    rec["patience"]["every3_last"] = [last["epoch"], last["stopped"]]

    # --- 6. a config that differs names its key
    path = os.path.join(tmp, "patience_8_5.pt")        # (by now the file of the finished run)
    mismatch = {}
    for key, value in (("lr", 1e-2), ("patience", 4), ("verbose", True)):
        c2 = dict(cfg, **{key: value})
        m = model(3)
        try:
            T.train_model(m, tr, va, c2, shuffle=False, engine=T.make_engine(m, c2, BATCH, n_batches),
                          evaluator=Stub([]), checkpoint=path, resume=True)
            mismatch[key] = ["ok", ""]
        except ValueError as e:
            mismatch[key] = ["ValueError", str(e)]
    rec["mismatch"] = mismatch

    # --- 7. library calls of a validated epoch with and without checkpointing
    real = N.lib()
    calls = []

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name in ("stdadk_last_error", "stdadk_abi_version"):
                return fn

            def call(*args):
                calls.append(name)
                return fn(*args)
            return call
    N.lib = lambda: Proxy()

    def trace(**kw):
        m = model()
        cfgt = {"lr": LR, "batch_size": BATCH, "grad_clip": 10.0, "epochs": 2, "warmup_epochs": 1, "scheduler": "cosine",
                "val_batch_size": BATCH, "verbose": False}
        e = T.make_engine(m, cfgt, BATCH, n_batches)
        del calls[:]
        T.train_model(m, tr, va, cfgt, shuffle=False, engine=e, **kw)
        return list(calls)
    rec["trace"] = {"off": trace(), "on": trace(checkpoint=os.path.join(tmp, "trace.pt"))}
    print("RECORD " + json.dumps(rec))


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("checkpoint"))
    env = dict(os.environ, STDADK_DRY_RUN="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), tmp], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RECORD ")][-1]
    return json.loads(line[len("RECORD "):])


@pytest.mark.parametrize("kind", ["fixed", "learn", "rank1"])
def test_round_trip_restores_every_buffer_in_place(rec, kind):
    """state_dict -> file -> load_state_dict into an engine built from another initialisation with another dropout
    seed: every buffer equal, no buffer moved, the announced batch dropped, both captured chains stale, the seed
    re-derived from the restored base seed and the LOADING engine's rank (rank 1 of 2 in `rank1`)."""
    r = rec["round_trip"][kind]
    assert r["different_before"] and r["rng_kept"] and r["extra"] == {"note": kind}
    wanted = {"flat", "m", "v", "ema", "step_dev", "loss_sum", "nonfinite", "lr_dev", "buffers.temporal_basis.centers",
              "buffers.temporal_basis.bandwidths"}
    wanted |= {"buffers.spatial_basis.centers_init", "basis_lr_dev"} if kind == "learn" else \
        {"buffers.spatial_basis.centers", "buffers.spatial_basis._bandwidths"}
    assert set(r["equal"]) == wanted
    assert all(r["equal"].values()), r["equal"]
    assert all(r["same_address"].values()), r["same_address"]
    assert r["prepared_none"] and r["graphs_stale"] == [True, True] and r["version_bumped"]
    seed, want, base_seed, rank = r["seed"]
    assert seed == want and base_seed == 5 and rank == (1 if kind == "rank1" else 0)
    assert r["counters"][:2] == r["counters"][2:] == [3, 3 * BATCH]
    assert r["rates"][:3] == [0.003, pytest.approx(0.003, rel=1e-7), 0.003]
    if kind == "learn":
        assert r["rates"][3:] == [0.0004, pytest.approx(0.0004, rel=1e-7), 0.0004]


@pytest.mark.parametrize("case,field", [("hidden", "layout"), ("dtype", "dtype"), ("dtype_back", "dtype"),
                                        ("ema_missing", "ema"), ("ema_extra", "ema"), ("grad_clip", "grad_clip"),
                                        ("format", "format"), ("weight_decay", "weight_decay"), ("world", "world")])
def test_load_refuses_and_names_the_field(rec, case, field):
    r = rec["refusals"]
    assert r["same"] == ["ok", ""]
    kind, text = r[case]
    assert kind == "ValueError" and text.startswith(field), (case, r[case])
    assert r["untouched"]


def test_one_call_and_split_steps_do_not_continue_each_other(rec):
    """With clipping on the one-call learnable step and the split calls sum the clip norm in another order: the door
    the step takes is part of the fingerprint."""
    kind, text = rec["refusals"]["step_call"]
    assert kind == "ValueError" and text.startswith("step_call"), rec["refusals"]["step_call"]


@pytest.mark.parametrize("which", ["swap_save", "swap_load"])
def test_state_is_refused_inside_a_swap_in_ema_pair(rec, which):
    """Between the two swaps the parameter buffer holds the shadow and the shadow the parameters: neither saved nor
    loaded there; after the second swap both work again."""
    inside, after = rec["refusals"][which]
    assert inside.startswith("RuntimeError") and "swap_in_ema" in inside and after == "ok", rec["refusals"][which]


def test_sharded_optimiser_is_not_covered(rec):
    for key in ("shard_save", "shard_load"):
        kind, text = rec["refusals"][key]
        assert kind == "NotImplementedError" and "shard_optimizer" in text, rec["refusals"][key]


def test_file_is_plain_data_and_survives_an_interrupted_write(rec):
    """The file loads under weights_only=True; when torch.save dies after writing, the checkpoint from before is still
    the one at the path and still loads (step_count 11, not 12)."""
    f = rec["file"]
    assert f["keys"] == ["engine", "extra", "format"] and f["engine_format"] == 1
    assert f["died"] and f["extra"] == {"n": 1} and f["step_count"] == 11


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("name", SCHED)
def test_learning_rates_across_a_cut_equal_the_reference(rec, name, cut):
    """`cut` epochs, death, a fresh model and engine resumed for the rest: every group's rate at every optimiser step --
    the host's number and the device scalar the kernels read -- and the history's lr column against the reference's
    own record (tests/golden/sched_*.npz), to the 1e-12 of the uninterrupted schedule test.  The cuts fall on the
    end of warm-up (1; 2 for sched_learn_now), the unfreezing epoch (2 of sched_learn), inside its ramp (3) and
    inside the cosine recursion (the rest)."""
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    r = rec["sched"][name][str(cut)]
    got = np.asarray(r["rates"], np.float64)
    host, device = got[:, 0::2], got[:, 1::2]
    assert host.shape == g["rates"].shape, (host.shape, g["rates"].shape)
    assert np.all(np.abs(host - g["rates"]) <= 1e-12 * np.abs(g["rates"])), np.argwhere(host != g["rates"])[:5]
    assert np.array_equal(device, host.astype(np.float32).astype(np.float64))       # what set_lr wrote
    lr = np.asarray(r["lr"], np.float64)
    assert lr.shape == g["lr"].shape and np.all(np.abs(lr - g["lr"]) <= 1e-12 * np.abs(g["lr"]))


def _same_run(a, b):
    """Histories, file names, CSV text and -- through the stub's stamps -- the CONTENTS of model_best.pt, the model and
    the device-side best state: every element is the number of the epoch the state is from."""
    for col in ("val_loss", "val_rmse", "train_loss", "lr"):
        x, y = a["hist"][col], b["hist"][col]
        assert len(x) == len(y) and all(p == q or (p != p and q != q) for p, q in zip(x, y)), (col, x, y)
    assert a["files"] == b["files"] == ["model_best.pt", "training_history.csv"]
    assert a["csv"] == b["csv"] and a["keys"] == b["keys"]
    assert a["best_is_model"] and b["best_is_model"]
    for what in ("best_file", "best_ema", "model", "shadow"):
        assert a[what] == b[what], (what, a[what], b[what])


@pytest.mark.parametrize("cut", [5, 6])
@pytest.mark.parametrize("epochs", [8, 10])
def test_best_state_and_patience_across_the_cut(rec, epochs, cut):
    """Validation losses 0.9 0.5 nan 0.7 0.4 0.45 0.41 0.6 [0.3 0.2], patience 3: best at epoch 5, early stop after the
    8th.  Cut after epoch 5 (the best epoch itself) and after epoch 6 (the patience counter at 1).  The file holds the
    best value, the counter and the best state (stamped 5); the resumed run stops after the 8th epoch with the
    uninterrupted run's history and files, and its model, model_best.pt and device-side best state are epoch 5's -- a
    forgotten best value would make epoch 6 or 7 best, a forgotten best tensor would be uninitialised memory.  With
    epochs = 10 the stop after the 8th can only come from the restored counter and best value: a counter restarted
    at 0 runs into epoch 9, whose 0.3 would be the new best.  Resuming the finished run takes no step and asks for
    no validation."""
    r = rec["patience"][str(epochs)]
    whole, resumed, again, saved = r["whole"], r[str(cut)], r[f"{cut}_again"], r[f"{cut}_saved"]
    nb = math.ceil(ROWS / BATCH)
    assert saved == {"epoch": cut, "stopped": False, "best_val": 0.4, "patience_counter": cut - 5, "has_best": True,
                     "best_state": {"distinct": [5.0], "sum": 5.0 * saved["best_state"]["numel"],
                                    "numel": saved["best_state"]["numel"]}}
    assert len(whole["hist"]["val_loss"]) == 8 and whole["steps"] == 8 * nb and whole["val_script_left"] == epochs - 8
    for what in ("best_file", "best_ema", "model"):
        assert whole[what]["distinct"] == [5.0] and whole[what]["sum"] == 5.0 * whole[what]["numel"], (what, whole[what])
    assert whole["shadow"]["distinct"] == [8.0]
    _same_run(whole, resumed)
    assert resumed["steps"] == 8 * nb and resumed["stub_calls"] == 8 - cut and resumed["val_script_left"] == epochs - 8
    _same_run(whole, again)
    assert again["steps"] == 8 * nb and again["stub_calls"] == 0


def test_resume_without_a_file_starts_at_epoch_zero(rec):
    _same_run(rec["patience"]["8"]["whole"], rec["patience"]["no_file"])
    assert rec["patience"]["every3_last"] == [8, True]          # 8 is no multiple of 3: the last epoch is always saved


def test_config_mismatch_names_the_key(rec):
    m = rec["mismatch"]
    assert m["lr"][0] == "ValueError" and "config['lr']" in m["lr"][1]
    assert m["patience"][0] == "ValueError" and "config['patience']" in m["patience"][1]
    assert m["verbose"] == ["ok", ""]


def test_checkpointing_makes_no_library_call(rec):
    t = rec["trace"]
    assert len(t["off"]) > 0 and t["on"] == t["off"]


if __name__ == "__main__":
    _record(sys.argv[1])
