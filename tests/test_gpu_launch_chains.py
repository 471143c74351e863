"""The dry-run launch log speaks for the real thing: for four cases of tests/test_launch_chains_cpu.py at 64 rows -- the
window one-call step, the materialising one-call step, the learnable fused step on the window path and the split
train_fwd_bwd with y_pred -- the names of the launches a real, profiled call makes equal the fixture's
(tests/golden/launch_chains.json), which was recorded without a device."""
import pytest
import torch

import test_launch_chains_cpu as chains

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    rec = chains.record("cuda:0", only=chains.GPU_CASES)
    torch.cuda.synchronize()
    return rec


@pytest.mark.parametrize("name", chains.GPU_CASES)
def test_real_launches_carry_the_dry_run_names(recorded, name):
    print(name, recorded[name])
    assert recorded[name] == chains.expected()[name]
