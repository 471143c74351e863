"""stnf.flat.FlatLayout on the CPU: every parameter's place in the flat buffers, for a learnable-knot delta-head model
and a plain one (no library call: flatten_parameters only moves storage)."""
import pytest
import torch

from stnf.flat import FlatLayout, flatten_parameters
from stnf.models import STInterpMLP

MODELS = {
    "learnable_delta": dict(k_spatial_centers=[25, 81], hidden_dims=[32, 16], output_dim=3, spatial_learnable=True,
                            use_delta_reparameterization=True),
    "plain": dict(k_spatial_centers=[25, 81], hidden_dims=[64, 64]),
}


@pytest.fixture(scope="module", params=sorted(MODELS))
def flattened(request):
    torch.manual_seed(0)
    m = STInterpMLP(p=0, k_temporal_centers=[10, 15], dropout=0.0, layernorm=True, **MODELS[request.param])
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    flat, lay = flatten_parameters(m)
    return m, before, flat, lay


def test_views_alias_the_parameters_and_keep_their_values(flattened):
    m, before, flat, lay = flattened
    assert isinstance(lay, FlatLayout) and flat.numel() == lay.numel and flat.dtype == torch.float32
    clone = flat.clone()
    first_w = m._body[0].weight
    assert [n for n, _, _ in lay.offsets] == [n for n, p in m.named_parameters() if p.requires_grad]
    for (n, p), (n2, o, k) in zip(m.named_parameters(), lay.offsets):
        assert n == n2 and lay.span(p) == (o, k) and k == p.numel()
        assert torch.equal(p.data, before[n]) and p.shape == before[n].shape       # flattening changed no value
        v = lay.view(flat, p)
        assert v.data_ptr() == p.data.data_ptr() == flat.data_ptr() + 4 * o        # the view aliases p.data
        c = lay.view(clone, p)
        assert c.data_ptr() == clone.data_ptr() + 4 * o
        if p is first_w:
            assert tuple(v.shape) == (p.shape[1], p.shape[0]) and v.is_contiguous()        # stored (in,out)
            assert torch.equal(v.t(), p.data) and torch.equal(c.t(), before[n])
        else:
            assert v.shape == p.shape and torch.equal(v, p.data) and torch.equal(c, before[n])


def test_spans_are_aligned_disjoint_and_padded(flattened):
    m, _, flat, lay = flattened
    end = 0
    for _, o, k in lay.offsets:
        assert o % 4 == 0 and (flat.data_ptr() + 4 * o) % 16 == 0                  # 16-byte aligned views
        assert o == end                                             # registration order, no gap but padding
        end = o + (k + 3) // 4 * 4
    assert end <= lay.numel < end + 4 and lay.numel % 4 == 0
    assert FlatLayout(m, pad_multiple=64).numel % 64 == 0 and FlatLayout(m, pad_multiple=64).offsets == lay.offsets


def test_hidden_weight_list_matches_the_linears(flattened):
    m, _, flat, lay = flattened
    lins = m._linears()
    assert lay.n_linears == len(lins)
    assert [l for l, _, _, _ in lay.hidden] == list(range(1, len(m.hidden_dims)))
    by_name = {n: o for n, o, _ in lay.offsets}
    names = {id(p): n for n, p in m.named_parameters()}
    for l, o, h, hp in lay.hidden:
        w = lins[l].weight
        assert (h, hp) == tuple(w.shape) == (m.hidden_dims[l], m.hidden_dims[l - 1])
        assert o == by_name[names[id(w)]] == lay.span(w)[0]
        assert torch.equal(flat[o:o + h * hp].view(h, hp), w.data)
    pairs, regions = lay.hidden_copies(lambda h, hp: (torch.empty(h, hp), torch.empty(hp, h)))
    assert len(pairs) == len(lins)
    assert [p is not None for p in pairs] == [0 < l < len(m.hidden_dims) for l in range(len(lins))]
    assert [(o, h, hp) for o, h, hp, _, _ in regions] == [(o, h, hp) for _, o, h, hp in lay.hidden]
    for (l, _, h, hp), (_, _, _, wb, wt) in zip(lay.hidden, regions):
        assert pairs[l][0] is wb and pairs[l][1] is wt and tuple(wb.shape) == (h, hp) and tuple(wt.shape) == (hp, h)
