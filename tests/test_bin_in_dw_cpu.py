"""Host side of the one-call step that announces its NEXT batch (stdadk_train_step_next_f32), without a GPU: with
STDADK_DRY_RUN=1 the library validates and plans -- the grid of the merged weight-gradient launch with its binning
workgroups included -- and launches nothing.  Checked here: the return code and `*next_binned` for both carriers of the
binning (STDADK_BIN_IN=dw|adam, read on every call), for sizes on both sides of what the carriers hold, and for a next
batch that fails its checks (nothing enqueued, `*next_binned == 0`).  stnf._native reads STDADK_DRY_RUN at import, so
this file is its own driver: run as a script in a child process it prints one JSON record, which the tests read."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 257, 1500, 4096, 6000]


def drive():
    for p in (ROOT, os.path.join(ROOT, "st-dadk_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("STDADK_DRY_RUN") == "1"
    import torch
    from stnf import _native as N
    from stnf.engine import TrainStep
    from stnf.models import STInterpMLP

    real = N.lib()
    seen = []

    class Proxy:
        """Keeps the return code and the value left in `*next_binned` of every stdadk_train_step_next_f32 call."""
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "stdadk_train_step_next_f32":
                return fn

            def call(*args):
                rc = fn(*args)
                seen.append((int(rc), int(args[-2]._obj.value)))
                return rc
            return call
    N.lib = lambda: Proxy()

    def engine(B, **kw):
        torch.manual_seed(0)
        m = STInterpMLP(p=kw.pop("p", 0), k_spatial_centers=[1024, 4096, 5184], k_temporal_centers=[10, 15, 45],
                        hidden_dims=[256, 256, 128], dropout=0.1, layernorm=True, output_dim=kw.pop("output_dim", 1)).train()
        eng = TrainStep(m, max_batch=B, ema_decay=0.99, **kw)
        assert eng._whole_step and eng.uses_window
        return eng

    def data(n, p=0, q=1):
        g = torch.Generator().manual_seed(1)
        return (torch.randn(n, p, generator=g) if p else None, torch.rand(n, 2, generator=g), torch.rand(n, generator=g),
                torch.randn(n, q, generator=g))

    def call(eng, X, c, t, y, B, nB, next_ws=None):
        idx = torch.arange(B - 1, -1, -1)
        nidx = torch.arange(nB)
        ws2 = torch.empty_like(eng.ws) if next_ws is None else next_ws
        del seen[:]
        try:
            took = eng._enqueue(X, c, t, y, B, B, idx=idx, ws=eng.ws, nxt=(nidx, ws2))
            err = None
        except RuntimeError as e:
            took, err = None, str(e)
        assert len(seen) == 1
        return {"took": took, "rc": seen[0][0], "next_binned": seen[0][1], "error": err}

    rec = {}
    for carrier in ("dw", "adam"):
        os.environ["STDADK_BIN_IN"] = carrier
        eng = engine(6000)
        X, c, t, y = data(6000)
        for nB in SIZES:
            # this step's batch is 4 096 rows (the merged weight-gradient launch), the next one nB
            rec[f"{carrier}/next{nB}"] = call(eng, X, c, t, y, 4096, nB)
        # a step of 6 000 rows (128 x 128 cells, still the merged launch) that announces 4 096
        rec[f"{carrier}/this6000"] = call(eng, X, c, t, y, 6000, 4096)
        # a next batch that fails: its workspace is too small
        rec[f"{carrier}/small_workspace"] = call(eng, X, c, t, y, 4096, 4096, next_ws=torch.empty(64))
        # workspaces that overlap: the weight-gradient launch must not carry it (the optimiser launch does)
        big = torch.empty(2 * eng.ws.numel() + 8)
        ws0, eng.ws = eng.ws, big[:eng.ws.numel()]
        rec[f"{carrier}/overlapping"] = call(eng, X, c, t, y, 4096, 4096, next_ws=big[4:4 + eng.ws.numel()])
        eng.ws = ws0
        for env in ("STDADK_NO_DW_ALL", "STDADK_NO_FUSED_TAIL"):
            os.environ[env] = "1"
            rec[f"{carrier}/{env}"] = call(eng, X, c, t, y, 4096, 1500)
            del os.environ[env]
        engq = engine(4096, p=3, output_dim=5, loss="pinball", quantile_levels=[0.05, 0.25, 0.5, 0.75, 0.95])
        Xq, cq, tq, yq = data(4096, p=3, q=5)
        rec[f"{carrier}/covariates_q5"] = call(engq, Xq, cq, tq, yq, 4096, 1500)
        engb = engine(4096, dtype="bf16")
        rec[f"{carrier}/bf16"] = call(engb, X, c, t, y, 4096, 4096)
    del os.environ["STDADK_BIN_IN"]
    print("RECORD " + json.dumps(rec))


@pytest.fixture(scope="module")
def rec():
    env = dict(os.environ, STDADK_DRY_RUN="1")
    for k in ("STDADK_BIN_IN", "STDADK_NO_DW_ALL", "STDADK_NO_FUSED_TAIL", "STDADK_BIN_WG", "STDADK_BIN_POS"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RECORD ")][-1]
    return json.loads(line[len("RECORD "):])


@pytest.mark.parametrize("carrier", ["dw", "adam"])
@pytest.mark.parametrize("nB", SIZES)
def test_next_batch_sizes(rec, carrier, nB):
    """Up to 4 096 rows (at most 64 x 64 cells) the step bins the next batch, whichever launch carries it; 6 000 rows
    the library declines with a clean return code and the caller prepares that batch itself."""
    r = rec[f"{carrier}/next{nB}"]
    assert r["rc"] == 0 and r["error"] is None
    assert r["next_binned"] == (1 if nB <= 4096 else 0) and r["took"] == (nB <= 4096)


@pytest.mark.parametrize("carrier", ["dw", "adam"])
@pytest.mark.parametrize("case", ["this6000", "overlapping", "STDADK_NO_DW_ALL", "STDADK_NO_FUSED_TAIL", "covariates_q5",
                                  "bf16"])
def test_next_batch_is_binned_whatever_the_step_runs(rec, carrier, case):
    """`*next_binned` keeps meaning "the next batch is binned": steps that do not run the merged weight-gradient launch,
    or may not let it write the next workspace, plan the optimiser launch with the binning instead."""
    r = rec[f"{carrier}/{case}"]
    assert r["rc"] == 0 and r["error"] is None and r["next_binned"] == 1 and r["took"] is True


@pytest.mark.parametrize("carrier", ["dw", "adam"])
def test_failing_next_batch_reports_nothing_binned(rec, carrier):
    """The next batch is validated before anything of the step is planned or enqueued."""
    r = rec[f"{carrier}/small_workspace"]
    assert r["rc"] < 0 and r["next_binned"] == 0 and r["took"] is None and "workspace" in r["error"]


if __name__ == "__main__":
    drive()
