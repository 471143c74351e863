"""Records tests/golden/adamw_stream_expected.npz: the outputs of the clip + AdamW + EMA launch for the order-sensitive
partials of adamw_stream_cases (family "spread"), per partial count.

The clip coefficient is a float32 sum of the partials, so its bits depend on the order of the additions.  The file holds
what the library computed BEFORE the partials' loads were unrolled (commit 'Python host layer: one flat layout, ...'),
recorded on an MI355X; tests/test_gpu_adamw_stream.py requires every later kernel to reproduce it bit for bit, which is
the proof that the order was kept.  Re-record only from a library whose order of additions is the reference:

    STDADK_LIB=/path/to/that/libstdadk.so python tests/golden/make_adamw_stream_expected.py

Needs the GPU.  A few KB of results, no program text.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE)),
           os.path.join(os.path.dirname(os.path.dirname(HERE)), "st-dadk_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from golden import adamw_stream_cases as sc               # noqa: E402
from golden import optim_cases as oc                      # noqa: E402

OUT = os.path.join(HERE, "adamw_stream_expected.npz")
OUTPUTS = ("p", "m", "v", "ema")


def run_parts_case(case, parts):
    """(outputs {p, m, v, ema}, arena, inputs) of `case` with hand-filled `parts`, NaNs behind them."""
    import torch
    import test_gpu_optim_elementwise as E
    import test_gpu_parity as T
    from stnf import _native as N
    d = T.dev()
    inp = oc.make_inputs(dict(case, clip=None))
    a = E.Arena(d, E._specs(case) + [("nanpad", sc.NAN_PAD, False)])
    E._load(a, inp)
    a.put("parts", parts)
    a.view("nanpad").fill_(float("nan"))
    parts_bits, pad_bits = a.get_bits("parts"), a.get_bits("nanpad")
    E._launch(N, a, case, d)
    a.check_sentinels()
    assert np.array_equal(a.get_bits("parts"), parts_bits) and np.array_equal(a.get_bits("nanpad"), pad_bits)
    torch.cuda.synchronize()
    return E._outputs(a, case), a, inp


def main():
    os.environ.pop("STDADK_ADAMW_BLOCKS", None)
    rec = {}
    for n_parts in sc.PART_COUNTS:
        case = sc.parts_case("spread", n_parts)
        got, _, _ = run_parts_case(case, sc.make_parts(case))
        for k in OUTPUTS:
            assert np.all(np.isfinite(got[k])), (n_parts, k)
            rec[f"{k}_{n_parts}"] = got[k].view(np.int32)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
