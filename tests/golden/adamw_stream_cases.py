"""Case tables of tests/test_gpu_adamw_stream.py: the float4 stream of the clip + AdamW + EMA launch (csrc/optim.hip) by
groups per thread, by the number of clip-norm partials, and by where the operand copies' regions lie in a thread's walk.

Numpy only and deterministic, like optim_cases.py (whose case dicts, inputs and bound these reuse).
"""
import numpy as np

from golden import optim_cases as oc

PARTS_U = 6                       # csrc/optim.hip: partials a thread has in flight at once

# ---- groups per thread -------------------------------------------------------------------------------------------
# Under STDADK_ADAMW_BLOCKS = b a thread walks float4 groups with stride 256 b.  n = 4 (k stride + r) + t gives threads
# with k and k + 1 groups around the edge r = -1, 0, 1 (so 1 .. 5 groups: odd and even counts, the last group of the
# walk partly filled, a prefetch that would reach one group past the end) and, with t = 3, a scalar tail behind them.
GROUP_BLOCKS = (1, 3)
GROUP_K = (1, 2, 3, 4)
GROUP_R = (-1, 0, 1)
GROUP_T = (0, 3)
GROUP_LAYOUTS = (("aligned", True), ("aligned", False), ("all", True), ("all", False))    # (alignment, EMA given)


def group_cases(blocks):
    """The cases of one forced grid: every size x aligned / shifted by 4 bytes x with / without an EMA buffer; steps,
    hyper-parameter sets and grad_mul alternate."""
    out, i = [], 0
    stride = 256 * blocks
    for k in GROUP_K:
        for r in GROUP_R:
            for t in GROUP_T:
                n = 4 * (k * stride + r) + t
                for align, ema in GROUP_LAYOUTS:
                    out.append(oc._case(f"stream_b{blocks}_k{k}_r{r}_t{t}_{align}_{'ema' if ema else 'noema'}", n, align,
                                        ema, oc.STEPS[i % len(oc.STEPS)], "wd" if i % 2 else "opt",
                                        0.25 if i % 3 == 0 else 1.0, None, blocks))
                    i += 1
    return out


# ---- partial counts --------------------------------------------------------------------------------------------------
PART_COUNTS = (1, 255, 256, 257, 256 * PARTS_U - 1, 256 * PARTS_U, 256 * PARTS_U + 1, 20 * 256 + 3)
PARTS_N = 69                      # elements of the stepped buffers: 17 groups and a scalar element
NAN_PAD = 256 * (PARTS_U + 2)     # NaNs behind the partials: further than any clamped or unrolled index could reach


def parts_case(family, n_parts):
    """family "int": small integers (their sum is exact in any order); "spread": magnitudes over 2^-20 .. 2^20, whose
    float32 sum depends on the order of the additions."""
    assert family in ("int", "spread")
    return oc._case(f"parts_{family}_{n_parts}", PARTS_N, "aligned", True, 3, "opt", 0.25, (None, n_parts))


def make_parts(case):
    family, n_parts = case["name"].split("_")[1], case["clip"][1]
    rs = np.random.RandomState(20261 + n_parts + (7 if family == "int" else 0))
    if family == "int":
        return rs.randint(100, 400, size=n_parts).astype(np.float32)         # sum <= 2.05 M < 2^24, norm > max_norm
    return np.ldexp(rs.uniform(1.0, 2.0, size=n_parts), rs.randint(-20, 21, size=n_parts)).astype(np.float32)


def thread_order_sum(parts, width=256):
    """float32 sum of the partials in the kernel's per-thread order (thread t adds t, t + width, ...), the threads'
    sums then added in index order -- NOT the kernel's tree behind the threads, which only the recorded outputs pin;
    this is for telling orders apart on the CPU."""
    acc = np.zeros(width, dtype=np.float32)
    for i in range(0, parts.size, width):
        row = parts[i:i + width]
        acc[:row.size] = acc[:row.size] + row
    s = np.float32(0.0)
    for x in acc:
        s = np.float32(s + x)
    return s


# ---- copies by position ----------------------------------------------------------------------------------------------
# n = 4 * 3 * 512 elements: under STDADK_ADAMW_BLOCKS = 2 every thread has three groups, under 1 six.  Two regions,
# 16 x 16 and 32 x 16, side by side at the start (a thread's first group), in the middle and at the end (its last).
COPY_BLOCKS = (1, 2)
COPY_N = 4 * 3 * 512
COPY_SHAPES = ((16, 16), (32, 16))
COPY_POSITIONS = {"start": 0, "middle": 4 * (512 + 100), "end": COPY_N - (16 * 16 + 32 * 16)}


def copy_regions(position):
    """[(offset, rows, cols)] of the two regions at `position`."""
    off, out = COPY_POSITIONS[position], []
    for rows, cols in COPY_SHAPES:
        out.append((off, rows, cols))
        off += rows * cols
    assert off <= COPY_N
    return out
