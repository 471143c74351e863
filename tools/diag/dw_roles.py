"""Per-role timing of ONE merged weight-gradient launch (dw_all_kernel) of the C2 train step (diagnostic build,
-DSTDADK_DIAG): first start and last end of the binning workgroups, of every grouped GEMM job, of the tall reduce jobs
and of the knot workgroups per level, and the chain length of a knot wave per level.
usage: STDADK_EXTRA_FLAGS=-DSTDADK_DIAG bash st-dadk_amd/csrc/build.sh && python tools/diag/dw_roles.py [B]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "st-dadk_amd")):
    sys.path.insert(0, p)
import torch
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
assert B <= 16384, "the stamp buffer is sized for the launches of small batches"
dev = torch.device("cuda:0")
NBLK = 65536
sf = torch.zeros(NBLK * 16, dtype=torch.int64, device=dev)
from stnf.models import STInterpMLP
from stnf.engine import TrainStep
torch.manual_seed(0)
m = STInterpMLP(k_spatial_centers=[1024, 4096, 5184], dropout=0.1).to(dev).train()
eng = TrainStep(m, lr=2e-2, weight_decay=5e-4, grad_clip=10.0, ema_decay=0.999, max_batch=B)
g = torch.Generator().manual_seed(1)
n = 64 * B
coords = torch.rand(n, 2, generator=g).to(dev); t = torch.rand(n, generator=g).to(dev); y = torch.randn(n, 1, generator=g).to(dev)
perm = torch.randperm(n, generator=g).to(dev)
sl = lambda i: perm[(i % 64) * B:(i % 64) * B + B]          # noqa: E731
for i in range(20):                                          # warm: clocks, caches, the one-call step with the next batch announced
    eng.step_indexed(coords, t, y, sl(i), next_idx=sl(i + 1))
torch.cuda.synchronize()
print(f"C2, fp32, {B} rows; times in us since the launch's first stamp")
os.environ["STDADK_DW_STAMPS"] = str(sf.data_ptr())
for rep in range(3):                                         # three launches, each read on its own
    sf.zero_()
    torch.cuda.synchronize()
    eng.step_indexed(coords, t, y, sl(20 + rep), next_idx=sl(21 + rep))
    torch.cuda.synchronize()
    w = sf.view(NBLK, 16).cpu()
    used = w[:, 0] > 0
    if not used.any():
        print("no stamps: not a -DSTDADK_DIAG build, or the step did not go through dw_all_kernel"); break
    role = w[:, 0] - 1
    t0 = int(w[used, 1].min())
    us = lambda x: (x.double() - t0) / 100.0                 # noqa: E731
    print(f"-- launch {rep}: {int(used.sum())} working workgroups of {int((w[:, 1] > 0).sum())} stamped, "
          f"launch {float(us(w[used, 2].max())):.2f} us first start to last end")
    print("   role                 blocks  block ids        first start  last start   first end    last end   median length")
    names = {0: "binning", 1: "tall reduce"}
    for r in sorted(set(role[used].tolist())):
        sel = used & (role == r)
        ids = sel.nonzero().flatten()
        nm = names.get(r, f"GEMM job {r - 10}" if r < 100 else f"knots level {r - 100}")
        s, e = us(w[sel, 1]), us(w[sel, 2])
        print(f"   {nm:20s} {int(sel.sum()):6d}  {int(ids.min()):5d}..{int(ids.max()):<5d}   {float(s.min()):10.2f}  {float(s.max()):10.2f}  "
              f"{float(e.min()):10.2f}  {float(e.max()):10.2f}   {float((e - s).median()):10.2f}")
    for r in sorted(set(role[used].tolist())):
        if r < 100:
            continue
        sel = used & (role == r)
        ws, we = w[sel][:, 4:12:2], w[sel][:, 5:12:2]
        ok = we > 0
        d = ((we - ws).double() / 100.0)[ok]
        print(f"   knot waves level {r - 100}: chain length median {float(d.median()):.2f} us, p90 {float(d.quantile(0.9)):.2f}, "
              f"max {float(d.max()):.2f}; last wave ends at {float(us(we[ok]).max()):.2f} us")
    last = int(w[used, 2].argmax())
    lr = int(role[used][last])
    print(f"   the launch's last workgroup to end: role {names.get(lr, 'GEMM job %d' % (lr - 10) if lr < 100 else 'knots level %d' % (lr - 100))}")
