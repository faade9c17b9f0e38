"""GPU: head_ops.linear_tokens on output widths that are no multiple of the GEMM's 8-column granularity (the padding lives
inside the Function), its weight cache, and the device seam every launch of heads / preprocess goes through (lib.call)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
F = torch.nn.functional


def relerr(got, ref):
    got, ref = got.float(), ref.float()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


def _linear_node(y):
    node = y.grad_fn
    while type(node).__name__ != "_HipLinearFnBackward":
        node = node.next_functions[0][0]
    return node


# pad 7; pad 5 with an odd row tail; pad 7 across two 8-column groups: the smallest shapes the dispatcher sends to HIP
@pytest.mark.parametrize("M,K,N", [(64, 8, 1), (65, 16, 3), (64, 72, 9)])
def test_linear_tokens_pads_inside_the_function(pkg, hiplib, M, K, N):
    """Unpadded shapes out; every result bitwise what the Function gives on explicitly zero-padded weight, bias and dy,
    sliced (the arithmetic F.pad + autograd's slice used to reach); within 8e-3 of fp32 on the bf16-rounded inputs."""
    ops = pkg.head_ops
    Np = (N + 7) // 8 * 8
    torch.manual_seed(M + K + N)
    lin = torch.nn.Linear(K, N).cuda()
    x = torch.randn(M, K, device="cuda").bfloat16().requires_grad_(True)
    dy = torch.randn(M, N, device="cuda").bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = ops.linear_tokens(x, lin.weight, lin.bias)
    wb = _linear_node(y).saved_tensors[1]
    assert wb.shape == (Np, K) and torch.equal(wb[:N], lin.weight.detach().bfloat16()) and not wb[N:].any()
    gx, gw, gb = torch.autograd.grad(y, [x, lin.weight, lin.bias], dy)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    assert gx.shape == (M, K) and gw.shape == (N, K) and gb.shape == (N,)

    wp = F.pad(lin.weight.detach(), (0, 0, 0, Np - N)).requires_grad_(True)
    bp = F.pad(lin.bias.detach(), (0, Np - N)).requires_grad_(True)
    xp = x.detach().clone().requires_grad_(True)
    yp = ops._HipLinearFn.apply(xp, wp, bp)
    px, pw, pb = torch.autograd.grad(yp, [xp, wp, bp], F.pad(dy, (0, Np - N)))
    assert yp.shape == (M, Np)
    assert torch.equal(y, yp[:, :N]) and torch.equal(gx, px) and torch.equal(gw, pw[:N]) and torch.equal(gb, pb[:N])

    xr = x.detach().float().requires_grad_(True)
    wr = lin.weight.detach().bfloat16().float().requires_grad_(True)
    yr = xr @ wr.t() + lin.bias
    rx, rw, rb = torch.autograd.grad(yr, [xr, wr, lin.bias], dy.float())
    errs = [relerr(y, yr), relerr(gx, rx), relerr(gw, rw), relerr(gb, rb)]
    print(f"M,K,N={M},{K},{N} relerr y,dX,dW,db = {errs}")
    assert max(errs) < 8e-3

    with torch.autocast("cuda", dtype=torch.bfloat16):
        y2 = ops.linear_tokens(x, lin.weight, lin.bias)
    assert _linear_node(y2).saved_tensors[1] is wb and torch.equal(y2, y)          # second forward: a cache hit
    with torch.no_grad():
        lin.weight.add_(0.5)                                                       # what optimizer.step() does
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y3 = ops.linear_tokens(x, lin.weight, lin.bias)
    wb3 = _linear_node(y3).saved_tensors[1]
    assert wb3 is not wb and torch.equal(wb3[:N], lin.weight.detach().bfloat16()) and not wb3[N:].any()


def test_mask_head_second_call_hits_the_cache(pkg, hiplib):
    """The decoder's 1-channel head passes conv.weight itself: one entry, re-used by the next call."""
    ops = pkg.head_ops
    torch.manual_seed(0)
    dec = pkg.heads.SegFormerMaskDecoder([16], embed_dim=8).cuda()
    x = torch.randn(2, 6, 6, 8, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a = dec._pointwise(dec.head, x)
        b = dec._pointwise(dec.head, x)
    assert a.shape == (2, 6, 6, 1) and torch.equal(a, b)
    assert _linear_node(a).saved_tensors[1] is _linear_node(b).saved_tensors[1] is ops._weights.get(dec.head.weight)[0]


def _recording_stub(monkeypatch, lib, symbol, status=0):
    seen = []

    def stub(*args):
        seen.append((torch.cuda.current_device(), args))
        return status
    monkeypatch.setattr(lib, symbol, stub)
    return seen


def test_seam_raises_naming_the_symbol(pkg, hiplib, monkeypatch):
    _recording_stub(monkeypatch, hiplib, "sgl_op_gate_mul", status=-1)
    with pytest.raises(pkg.lib.SglError, match="sgl_op_gate_mul: bad shape"):
        pkg.lib.call("sgl_op_gate_mul", torch.device("cuda", torch.cuda.current_device()), 0, 0, 0, 0, 0)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_seam_launches_on_the_operands_device(pkg, hiplib, monkeypatch):
    """No kernel of the library runs: a recording stub stands in for the symbol.  With cuda:0 current and a side stream
    current on cuda:1, a call for cuda:1 operands runs under cuda:1's guard with cuda:1's stream as its last argument, and
    cuda:0 is current again afterwards: directly, through head_ops.gate_mul and through preprocess.resize_normalize."""
    dev1 = torch.device("cuda:1")
    side = torch.cuda.Stream(device=dev1)
    gate = torch.randn(4096, device=dev1)
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev1)
    calls = {"direct": ("sgl_op_gate_mul", lambda: pkg.lib.call("sgl_op_gate_mul", dev1, 1, 2, 3, 4, 0)),
             "gate_mul": ("sgl_op_gate_mul", lambda: pkg.head_ops.gate_mul(gate, gate)),
             "resize_normalize": ("sgl_op_preprocess", lambda: pkg.preprocess.resize_normalize(img, 4))}
    for name, (symbol, fn) in calls.items():
        seen = _recording_stub(monkeypatch, hiplib, symbol)
        with torch.cuda.stream(side), torch.cuda.device(0):
            want = torch.cuda.current_stream(1).cuda_stream
            assert torch.cuda.current_device() == 0 and want == side.cuda_stream != torch.cuda.default_stream(1).cuda_stream
            fn()
            assert torch.cuda.current_device() == 0, name
        assert len(seen) == 1, name
        device, args = seen[0]
        assert device == 1 and args[-1] == want, name
