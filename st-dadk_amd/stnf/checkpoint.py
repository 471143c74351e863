"""Checkpoints of a training run: `TrainStep.state_dict()` plus whatever the caller drives the engine with (`extra`:
the epoch driver's schedule, best state, history and permutation RNG), in one file that a later process continues from
bit for bit (`TrainStep.load_state_dict`).

The file is written next to its destination and moved over it in one step, so a write that is interrupted -- the very
time limit or pre-emption a checkpoint is for -- leaves the previous checkpoint as it was.  It holds tensors, numbers,
strings, lists and dicts only and is read with `weights_only=True`: loading one executes nothing."""
import os

import torch

FORMAT = 1


def save_checkpoint(path, engine, extra=None):
    """Write `engine.state_dict()` and `extra` (tensors, numbers, strings, lists, dicts) to `path`.  One writer per
    path: of several replicated data-parallel ranks one saves (they would share `path + ".tmp"`), all of them load."""
    path = str(path)
    tmp = path + ".tmp"
    torch.save({"format": FORMAT, "engine": engine.state_dict(), "extra": extra}, tmp)
    os.replace(tmp, path)


def read_checkpoint(path):
    """The file's contents, {"format", "engine", "extra"}, on the host; nothing is loaded anywhere."""
    ck = torch.load(str(path), map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or ck.get("format") != FORMAT:
        raise ValueError(f"format: {ck.get('format') if isinstance(ck, dict) else type(ck).__name__!r} is not a "
                         f"checkpoint format this version reads ({FORMAT})")
    return ck


def load_checkpoint(path, engine):
    """Load the file into `engine` (`TrainStep.load_state_dict`: refusals are ValueErrors naming the field) and return
    its `extra`."""
    ck = read_checkpoint(path)
    engine.load_state_dict(ck["engine"])
    return ck["extra"]
