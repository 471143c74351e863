"""The flat parameter storage of an engine (stnf.engine.TrainStep): where every parameter lives in it, and the two
small tools everything that keeps state derived from it shares -- the keyed descriptor cache and the counter that
tells derived copies the parameters were rewritten."""
import torch


class FlatLayout:
    """Where every trainable parameter of `model` lives in the flat fp32 buffers -- parameters, gradient, Adam
    moments, EMA shadow and any clone of them share it.  Each parameter is padded to a multiple of 4 floats, so every
    view is 16-byte aligned; with `transpose_first` the first Linear's weight is STORED (in,out) row-major, the layout
    the window kernels gather rows from.  The length `numel` is rounded up to `pad_multiple` floats (equal shards of a
    sharded optimiser).
      offsets   [(name, offset, numel)] in named_parameters() order
      hidden    [(layer, offset, h, hp)] of the hidden Linear weights after the first (Linear index, shape (h, hp))"""

    def __init__(self, model, transpose_first=True, pad_multiple=4):
        self.params = [p for _, p in model.named_parameters() if p.requires_grad]
        self.offsets, self._spans, total = [], {}, 0
        for n, p in model.named_parameters():
            if p.requires_grad:
                self.offsets.append((n, total, p.numel()))
                self._spans[id(p)] = (total, p.numel())
                total += (p.numel() + 3) // 4 * 4
        self.numel = (total + pad_multiple - 1) // pad_multiple * pad_multiple
        self.first_w = model._body[0].weight if transpose_first else None
        lins = model._linears()
        self.n_linears = len(lins)
        self.hidden = [(l, self.span(lins[l].weight)[0]) + tuple(lins[l].weight.shape)
                       for l in range(1, len(model.hidden_dims))]

    def span(self, p):
        """(offset, numel) of parameter `p`."""
        return self._spans[id(p)]

    def view(self, buf, p):
        """The view of `p` in a flat-shaped buffer: p's shape, the first weight as it is stored, (in,out)."""
        o, k = self._spans[id(p)]
        if p is self.first_w:
            return buf[o:o + k].view(p.shape[1], p.shape[0])
        return buf[o:o + k].view(p.shape)

    def hidden_copies(self, alloc):
        """Operand copies of the hidden weights after the first: `alloc(h, hp)` -> (copy, transposed copy) per weight.
        Returns (the pairs by Linear index, None where there is none; the regions [(offset, h, hp, copy, copy_t)] a
        stdadk_bf16_shadow table is made from)."""
        pairs, regions = [None] * self.n_linears, []
        for l, o, h, hp in self.hidden:
            pairs[l] = tuple(alloc(h, hp))
            regions.append((o, h, hp) + pairs[l])
        return pairs, regions


def flatten_parameters(model, transpose_first=True, pad_multiple=4):
    """Move every trainable parameter of `model` into one flat fp32 buffer laid out by `FlatLayout` (the parameters
    become views, so state_dict()/checkpoints keep their names and shapes; `model.mlp[0].weight` becomes the .t() view
    of its stored (in,out) form: same values, shape (out,in)).  Returns (flat, layout)."""
    lay = FlatLayout(model, transpose_first, pad_multiple)
    flat = torch.zeros(lay.numel, device=lay.params[0].device, dtype=torch.float32)
    for p in lay.params:
        v = lay.view(flat, p)
        if p is lay.first_w:
            v.copy_(p.data.t())
            p.data = v.t()
        else:
            v.copy_(p.data)
            p.data = v
    return flat, lay


class Cached:
    """Descriptors kept per slot in `self._cache` and rebuilt when the key they were built from changes."""

    def _cached(self, slot, key, build, *args):
        hit = self._cache.get(slot)
        if hit is None or hit[0] != key:
            hit = self._cache[slot] = (key, build(*args))
        return hit[1]


def _bump_engine_version(model):
    """The parameters were rewritten by something autograd's version counters do not see (kernels writing through raw
    pointers, whole-buffer copies): everything that caches tensors derived from them -- a Predictor's output layer of
    the delta head or transposed W0, an engine's operand copies -- watches this counter."""
    model._engine_version = getattr(model, "_engine_version", 0) + 1
