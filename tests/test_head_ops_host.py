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


def _assert_current(cache, p):
    """Both operands the cache hands out are casts of the parameter as it is NOW."""
    w, wt = cache.get(p, want_t=True)
    want = p.detach().flatten(1).bfloat16()
    n = want.shape[0]
    assert torch.equal(w[:n], want) and not w[n:].any(), "stale W"
    assert torch.equal(wt, w.t()) and wt.is_contiguous(), "stale transpose"


def _route_inplace(lin):
    with torch.no_grad():
        lin.weight.add_(0.75)


def _route_detached_inplace(lin):
    lin.weight.detach().mul_(-1.5)


def _route_load_state_dict(lin):
    lin.load_state_dict({k: v * 2.0 + 1.0 for k, v in lin.state_dict().items()})


def _route_broadcast_write(lin):
    import __graft_entry__ as g
    ddp = g.load_package().ddp
    ts = [*lin.parameters()]
    ddp.write_flat(ts, torch.cat([t.detach().reshape(-1) for t in ts]) * 3.0 - 1.0)


def _route_data_swap(lin):
    lin.weight.data = lin.weight.data * 0.5 + 2.0


def _route_channels_last(lin):
    lin.to(memory_format=torch.channels_last)
    with torch.no_grad():
        lin.weight.mul_(1.25)


ROUTES = [_route_inplace, _route_detached_inplace, _route_load_state_dict, _route_broadcast_write, _route_data_swap,
          _route_channels_last]


def test_weight_cache_follows_every_tracked_write_route(pkg):
    """Each route that writes a weight, after both operands (W and the transpose the backward reads) were cached: what
    the cache returns next is the cast of the new values, the transpose included.  A 9-row Linear (padded to 16) and the
    decoder's (out, in, 1, 1) convolution weight."""
    for route in ROUTES:
        for make in (lambda: torch.nn.Linear(24, 9), lambda: torch.nn.Conv2d(16, 8, 1)):
            torch.manual_seed(7)
            lin = make()
            cache = pkg.head_ops.WeightCache()
            _assert_current(cache, lin.weight)
            before = lin.weight.detach().clone()
            route(lin)
            assert not torch.equal(before, lin.weight.detach()), route.__name__      # the route did write
            _assert_current(cache, lin.weight)
            assert len(cache) == 1, route.__name__


def test_weight_cache_follows_a_data_pointer_swap_and_back(pkg):
    """The reference's EMA helper (cifake_binary_classifier.py:227-236) swaps ``param.data`` for the average and back: the
    version stays, the address moves, and each side gets its own cast."""
    cache = pkg.head_ops.WeightCache()
    p = _param(9, 24, 11)
    live, avg = p.data, torch.full_like(p.data, 0.3)
    _assert_current(cache, p)
    p.data = avg
    assert p._version == 0
    _assert_current(cache, p)
    assert torch.equal(cache.get(p)[0][:9], avg.bfloat16())
    p.data = live
    _assert_current(cache, p)


def test_weight_cache_sees_changed_averages_at_the_second_ema_swap(pkg):
    """apply_shadow -> read -> restore -> the averages change (a stand-alone update(), a checkpoint loaded into
    ``shadow``) -> apply_shadow -> read.  The averages sit at fixed addresses, so the second swap shows the address of the
    first; only the version ``apply_shadow`` bumps tells the two apart."""
    torch.manual_seed(5)
    lin = torch.nn.Linear(24, 9)
    ema = pkg.ExponentialMovingAverage(lin, decay=0.5)
    cache = pkg.head_ops.WeightCache()
    _assert_current(cache, lin.weight)
    ema.apply_shadow()
    first_key = (lin.weight._version, lin.weight.data_ptr())
    _assert_current(cache, lin.weight)
    ema.restore()
    _assert_current(cache, lin.weight)
    ema.shadow["weight"].mul_(0.5).add_(1.0)          # what update() does to the average, with no parameter step
    ema.apply_shadow()
    assert lin.weight.data_ptr() == first_key[1] and lin.weight._version != first_key[0]
    _assert_current(cache, lin.weight)
    assert torch.equal(cache.get(lin.weight)[0][:9], ema.shadow["weight"].bfloat16())
    ema.restore()
    _assert_current(cache, lin.weight)


def test_deepcopy_of_a_cached_module_gets_entries_of_its_own(pkg):
    import copy
    ops = pkg.head_ops
    torch.manual_seed(2)
    lin = torch.nn.Linear(24, 9)
    before = len(ops._weights)
    w = ops._weights.get(lin.weight, want_t=True)
    twin = copy.deepcopy(lin)
    with torch.no_grad():
        twin.weight.mul_(2.0)
    w2 = ops._weights.get(twin.weight, want_t=True)
    assert w2[0] is not w[0] and w2[1] is not w[1] and len(ops._weights) == before + 2
    assert torch.equal(w2[0][:9], twin.weight.detach().bfloat16()) and torch.equal(w2[1], w2[0].t())
    assert ops._weights.get(lin.weight)[0] is w[0] and torch.equal(w[0][:9], lin.weight.detach().bfloat16())
    assert ops.invalidate_weights(lin) == 1 and ops.invalidate_weights(twin) == 1


def test_invalidate_weights_is_the_way_out_after_an_untracked_write(pkg):
    """An in-place write through ``p.data`` moves neither the version nor the address: the cache cannot see it (INTEGRATION.md
    lists it as untracked), and ``head_ops.invalidate_weights(module)`` drops the module's entries by hand."""
    ops = pkg.head_ops
    torch.manual_seed(3)
    dec = torch.nn.Sequential(torch.nn.Linear(24, 9), torch.nn.Sequential(torch.nn.Conv2d(16, 8, 1)))
    other = torch.nn.Linear(8, 8)
    ws = [p for p in dec.parameters() if p.dim() > 1]
    for p in (*ws, other.weight):
        ops._weights.get(p, want_t=True)
    kept = ops._weights.get(other.weight)[0]
    for p in ws:
        key = (p._version, p.data_ptr())
        p.data.mul_(3.0)
        assert (p._version, p.data_ptr()) == key
        assert not torch.equal(ops._weights.get(p)[0][:p.shape[0]], p.detach().flatten(1).bfloat16())    # stale, as documented
    assert ops.invalidate_weights(dec) == 2            # the two weights; the biases were never cached
    for p in ws:
        _assert_current(ops._weights, p)
    assert ops._weights.get(other.weight)[0] is kept   # another module's entry is left alone
    assert ops.invalidate_weights(dec) == 2 and ops.invalidate_weights(dec) == 0
    ops.invalidate_weights(other)


def test_sgl_heads_linear_is_gone_from_the_package(pkg):
    """SGL_HEADS_LINEAR=torch used to reroute the decoder's GEMMs at import.  With it set in the environment of an
    interpreter that imports the package nothing may read it any more: the name does not occur in the package's source."""
    root = os.path.dirname(os.path.abspath(pkg.__file__))
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".h", "Makefile")):
                with open(os.path.join(d, f), errors="replace") as fh:
                    assert "SGL_HEADS_LINEAR" not in fh.read(), os.path.join(d, f)
