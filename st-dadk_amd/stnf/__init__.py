"""stnf — MI355X (gfx950) build of ST-DADK's spatio-temporal interpolation hot path.

Same import surface as the reference package for the path that is built here
(`stnf.models`, `stnf.dataio.kaust_loader.load_kaust_csv_single`, `stnf.utils`); the arithmetic
runs in libstdadk.so (hand-written HIP).  Put `st-dadk_amd/` on PYTHONPATH and the reference's
`scripts/train_st_interp.py` imports this package instead of its own.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # the epoch driver and the evaluator, imported on first use (they pull in torch and the native library)
    if name in ("train_model", "evaluate_model"):
        from . import training
        return getattr(training, name)
    if name == "Evaluator":
        from .evaluation import Evaluator
        return Evaluator
    raise AttributeError(f"module 'stnf' has no attribute '{name}'")
