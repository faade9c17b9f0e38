"""CPU (no GPU, no library): the weight cache of head_ops on CPU tensors, and the retired SGL_HEADS_LINEAR switch."""
import gc
import os

import torch


def _param(n, k, seed=0):
    return torch.nn.Parameter(torch.randn(n, k, generator=torch.Generator().manual_seed(seed)))


def test_weight_cache_hits_on_the_same_parameter_and_rebuilds_on_a_new_version(pkg):
    cache = pkg.head_ops.WeightCache()
    p = _param(16, 8)
    w, wt = cache.get(p)
    assert wt is None and w.dtype == torch.bfloat16 and w.is_contiguous()
    assert torch.equal(w, p.detach().bfloat16())
    assert cache.get(p)[0] is w and len(cache) == 1
    with torch.no_grad():
        p.mul_(3.0)                         # what an optimizer step does: bumps p._version
    w2, _ = cache.get(p)
    assert w2 is not w and torch.equal(w2, p.detach().bfloat16()) and len(cache) == 1
    assert cache.get(p)[0] is w2


def test_weight_cache_pads_rows_to_a_multiple_of_eight(pkg):
    cache = pkg.head_ops.WeightCache()
    one, nine = _param(1, 8, 1), _param(9, 8, 2)
    w1, w9 = cache.get(one)[0], cache.get(nine)[0]
    assert w1.shape == (8, 8) and torch.equal(w1[:1], one.detach().bfloat16()) and not w1[1:].any()
    assert w9.shape == (16, 8) and torch.equal(w9[:9], nine.detach().bfloat16()) and not w9[9:].any()
    conv = torch.nn.Conv2d(8, 1, 1)         # the mask head: the cache takes the (out, in) view of (out, in, 1, 1)
    wc = cache.get(conv.weight)[0]
    assert wc.shape == (8, 8) and torch.equal(wc[0], conv.weight.detach().view(8).bfloat16()) and not wc[1:].any()


def test_weight_cache_builds_the_transpose_on_demand_and_keeps_it(pkg):
    cache = pkg.head_ops.WeightCache()
    p = _param(9, 24, 3)
    w, none = cache.get(p)
    assert none is None
    w_again, wt = cache.get(p, want_t=True)
    assert w_again is w and wt.shape == (24, 16) and wt.is_contiguous() and torch.equal(wt, w.t())
    assert cache.get(p, want_t=True)[1] is wt and cache.get(p)[1] is wt
    with torch.no_grad():
        p.add_(1.0)
    assert cache.get(p)[1] is None          # a rebuilt entry starts without its transpose


def test_weight_cache_entry_dies_with_its_parameter_and_never_aliases_the_next_one(pkg):
    cache = pkg.head_ops.WeightCache()
    p = _param(8, 8, 4)
    first = cache.get(p)[0].clone()
    assert len(cache) == 1
    del p
    gc.collect()
    assert len(cache) == 0
    q = _param(8, 8, 5)                     # same shape, allocated right after: may reuse the address and the id()
    got = cache.get(q)[0]
    assert torch.equal(got, q.detach().bfloat16()) and not torch.equal(got, first)
    assert len(cache) == 1


def test_sgl_heads_linear_is_gone_from_the_package(pkg):
    """SGL_HEADS_LINEAR=torch used to reroute the decoder's GEMMs at import.  With it set in the environment of an
    interpreter that imports the package nothing may read it any more: the name does not occur in the package's source."""
    root = os.path.dirname(os.path.abspath(pkg.__file__))
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".h", "Makefile")):
                with open(os.path.join(d, f), errors="replace") as fh:
                    assert "SGL_HEADS_LINEAR" not in fh.read(), os.path.join(d, f)
