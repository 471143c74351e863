"""Event timing of the AdamW+EMA kernel alone under the conditions it meets in the headline step: a C2-sized flat
buffer, ~1 300 clip-norm partials, operand-copy regions at the end of the buffer.

    python tools/bench_adamw_step_like.py [n_parts] [copies|nocopies]        (STDADK_LIB selects the library)
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "st-dadk_amd")):
    sys.path.insert(0, p)
import torch
from stnf import _native as N
n = 2756100
n_parts = int(sys.argv[1]) if len(sys.argv) > 1 else 1304
copies = (sys.argv[2] == "copies") if len(sys.argv) > 2 else True
dev = torch.device("cuda:0")
p, g, m, v, e = (torch.randn(n, device=dev) for _ in range(5))
v.abs_()
parts = torch.rand(n_parts, device=dev)
sh = None
if copies:
    regs, off = [], n - 4 - (256 * 256 + 256 * 128)
    off -= off % 4
    for rows, cols in ((256, 256), (128, 256)):
        regs.append((off, rows, cols, torch.zeros(rows * cols, dtype=torch.bfloat16, device=dev),
                     torch.zeros(rows * cols, dtype=torch.bfloat16, device=dev)))
        off += rows * cols
    sh = N.make_bf16_shadow(regs)
def run():
    N.adamw_ema(p, g, m, v, e, 1e-3, (0.9, 0.999), 1e-8, 5e-4, 3, max_norm=10.0, sumsq_parts=parts, ema_decay=0.999, shadow=sh)
for _ in range(5): run()
torch.cuda.synchronize()
N.profile_enable(True)
for _ in range(100): run()
recs = N.profile_collect(); N.profile_enable(False)
ts = sorted(ms for nm, ms in recs if "adamw" in nm)
print(f"adamw n_parts={n_parts} copies={copies}: median {ts[len(ts)//2]*1e3:.2f} us  mean {sum(ts)/len(ts)*1e3:.2f} us  min {ts[0]*1e3:.2f}")
