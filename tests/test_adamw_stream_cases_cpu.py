"""The case tables of tests/test_gpu_adamw_stream.py on the CPU: the sizes reach the group counts they are meant to, the
order-sensitive partials do tell orders of addition apart, and the recorded outputs have the tables' shape."""
import os

import numpy as np

from golden import adamw_stream_cases as sc
from golden import make_adamw_stream_expected as mk
from golden import optim_cases as oc


def test_sizes_give_one_to_five_groups_per_thread():
    for blocks in sc.GROUP_BLOCKS:
        stride, counts, tails = 256 * blocks, set(), set()
        for case in sc.group_cases(blocks):
            n4 = case["n"] // 4
            counts |= {-(-(n4 - t) // stride) for t in (0, stride - 1) if n4 > t}     # first and last thread
            tails.add(case["n"] % 4)
        assert counts == {1, 2, 3, 4, 5}, (blocks, counts)
        assert tails == {0, 3}


def test_spread_partials_tell_orders_apart():
    """With several partials per thread (the counts around 256 PARTS_U and beyond) the float32 sum in the kernel's
    per-thread order differs from the sum in index order: a kernel that added them in another order would change the
    coefficient's bits.  (Up to 257 partials a thread has one entry, thread 0 at most two: nothing to re-order.)"""
    for n_parts in sc.PART_COUNTS:
        parts = sc.make_parts(sc.parts_case("spread", n_parts))
        assert parts.dtype == np.float32 and parts.size == n_parts and np.all(parts > 0)
        seq = np.float32(0.0)
        for x in parts:
            seq = np.float32(seq + x)
        if n_parts >= 256 * sc.PARTS_U - 1:
            assert sc.thread_order_sum(parts) != seq, n_parts
            assert float(np.sqrt(seq)) > oc.HYPER["opt"]["max_norm"]          # the coefficient is below 1: it matters


def test_integer_partials_sum_exactly():
    for n_parts in sc.PART_COUNTS:
        parts = sc.make_parts(sc.parts_case("int", n_parts))
        assert np.all(parts == np.round(parts)) and float(parts.astype(np.float64).sum()) < 2.0 ** 24
        assert float(sc.thread_order_sum(parts)) == float(parts.astype(np.float64).sum())


def test_recorded_outputs_match_the_tables():
    assert os.path.getsize(mk.OUT) < 64 * 1024
    rec = np.load(mk.OUT)
    assert sorted(rec.files) == sorted(f"{k}_{n}" for k in mk.OUTPUTS for n in sc.PART_COUNTS)
    for name in rec.files:
        assert rec[name].dtype == np.int32 and rec[name].shape == (sc.PARTS_N,)
        assert np.all(np.isfinite(rec[name].view(np.float32)))


def test_copy_regions_lie_in_first_middle_and_last_groups():
    for blocks in sc.COPY_BLOCKS:
        stride, last = 256 * blocks, sc.COPY_N // 4 // (256 * blocks) - 1
        k = {pos: {(off // 4) // stride for off, _, _ in sc.copy_regions(pos)} for pos in sc.COPY_POSITIONS}
        assert k["start"] == {0} and k["end"] == {last} and all(0 < x < last for x in k["middle"]), (blocks, k)
