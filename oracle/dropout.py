"""The dropout keep-mask contract of include/stdadk.h ("Dropout keep-masks"), restated on the CPU.  TEST
INFRASTRUCTURE ONLY; numpy only, written from the header's text and never calling the library.

  step seed   s   = (drop_seed + step * 0x9E3779B97F4A7C15) mod 2^64
  row key     k   = mix32(s ^ (0x9E3779B97F4A7C15 * (layer + 1) mod 2^64) ^ (row * 0xD1B54A32D192ED03 mod 2^64))
  pair        j   = (col & 63) | ((col >> 7) << 6)            columns c and c + 64 of a 128-column block share j
  hash        h   = fin32(k ^ (j * 0x9E3779B1 mod 2^32))
  bits        v   = h >> 16 if col & 64 else h & 0xffff
  keep            = v >= ceil(float32(p) * 65536);  kept values are scaled by 1 / (1 - p)

Two implementations: a vectorised one (uint64 / uint32 arrays, wrapping arithmetic) that the tests use, and a scalar
one in plain Python integers with explicit masks (`*_scalar`) that tests/test_dropout_cases_cpu.py holds the first
against.
"""
import numpy as np

from . import stdadk_oracle as orc

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
PHI64 = 0x9E3779B97F4A7C15
ROW_MUL = 0xD1B54A32D192ED03
PAIR_MUL = 0x9E3779B1


# ------------------------------------------------------------------------------------------------ scalar
def step_seed(seed, step):
    """Seed of one step: drop_seed + step_dev[0] * PHI64 mod 2^64 (Python ints)."""
    return (int(seed) + int(step) * PHI64) & M64


def threshold(p):
    """ceilf(p * 65536) with p and the product in float32 (the product by a power of two is exact)."""
    return int(np.ceil(np.float32(p) * np.float32(65536.0)))


def _mix32_scalar(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x & M32


def hash_scalar(seed, step, layer, row, col):
    """The 32-bit hash that decides element (row, col) of `layer` (and its partner column col ^ 64)."""
    s = step_seed(seed, step)
    k = _mix32_scalar(s ^ ((PHI64 * (int(layer) + 1)) & M64) ^ ((int(row) * ROW_MUL) & M64))
    col = int(col)
    pair = (col & 63) | ((col >> 7) << 6)
    h = (k ^ ((pair * PAIR_MUL) & M32)) & M32
    h ^= h >> 16
    h = (h * 0x21F0AAAD) & M32
    h ^= h >> 15
    h = (h * 0x735A2D97) & M32
    h ^= h >> 15
    return h


def keep_scalar(seed, step, layer, row, col, p):
    h = hash_scalar(seed, step, layer, row, col)
    bits = (h >> 16) if (int(col) >> 6) & 1 else (h & 0xFFFF)
    return bits >= threshold(p)


# ------------------------------------------------------------------------------------------------ vectorised
def _u64(x):
    return np.uint64(int(x) & M64)


def hash_bits(seed, step, layer, rows, h):
    """(hash uint32 [len(rows), h], 16 deciding bits uint32 [len(rows), h]) of one layer."""
    rows = np.asarray(rows)
    assert rows.ndim == 1 and rows.dtype.kind in "iu" and (rows.size == 0 or rows.min() >= 0)
    with np.errstate(over="ignore"):
        x = _u64(step_seed(seed, step)) ^ _u64(PHI64 * (int(layer) + 1)) ^ (rows.astype(np.uint64) * _u64(ROW_MUL))
        x ^= x >> np.uint64(33)
        x *= _u64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= _u64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
        key = (x & _u64(M32)).astype(np.uint32)
        col = np.arange(int(h), dtype=np.uint32)
        pair = (col & np.uint32(63)) | ((col >> np.uint32(7)) << np.uint32(6))
        v = key[:, None] ^ (pair * np.uint32(PAIR_MUL))[None, :]
        v ^= v >> np.uint32(16)
        v *= np.uint32(0x21F0AAAD)
        v ^= v >> np.uint32(15)
        v *= np.uint32(0x735A2D97)
        v ^= v >> np.uint32(15)
    high = ((col >> np.uint32(6)) & np.uint32(1)).astype(bool)
    bits = np.where(high[None, :], v >> np.uint32(16), v & np.uint32(0xFFFF))
    return v, bits


def keep_mask(seed, step, layer, rows, h, p):
    """bool [len(rows), h]: element (i, c) is kept in `layer` (0-based hidden layer) of the step that reads
    step_dev[0] == step, for the row whose key is rows[i]."""
    return hash_bits(seed, step, layer, rows, h)[1] >= np.uint32(threshold(p))


def keep_masks(seed, step, rows, hidden_dims, p):
    """The masks of every hidden layer, as orc.mlp_forward(drop_masks=...) takes them."""
    return [keep_mask(seed, step, l, rows, h, p) for l, h in enumerate(hidden_dims)]


# ------------------------------------------------------------------------------------------------ row keys
def window_order(coords, cell_side):
    """Caller order -> window-path order: the stable sort by cell key on the cell_side x cell_side binning grid
    (sorted position -> caller row; the permutation N.bin_obs returns)."""
    return np.argsort(orc.cell_keys(coords, cell_side), kind="stable")


def window_rows(coords, cell_side):
    """Row key of every caller row on the window path: its SORTED position."""
    perm = window_order(coords, cell_side)
    pos = np.empty(len(perm), dtype=np.int64)
    pos[perm] = np.arange(len(perm), dtype=np.int64)
    return pos
