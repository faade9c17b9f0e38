"""The one attention runner of the GPU kernel tests (tests/test_kernel_edges_gpu.py, tests/test_kernels_gpu.py,
tests/test_fp16_gpu.py, tests/gen_attn_digests.py): forward and backward through the C ABI with every output inside guard
bands, and the two references the tests compare with.  `Guarded` and the small call helpers live here too, so that the
test modules can share them without importing one another."""
import torch

import kernel_ref as kr
from kernel_ref import BF16X3, F32

DEV = "cuda"


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def ok(st):
    assert st == 0, f"C ABI status {st}"


def tdt_of(dtype):
    return kr.TORCH_DT[dtype]


def rup(x, m):
    return (x + m - 1) // m * m


class Guarded:
    """A [rows, width] output inside one allocation of (rows + 2 G) x ld elements: everything but the body holds a
    sentinel bit pattern, the body NaN (or `prior`)."""
    G = 16

    def __init__(self, rows, width, ld, tdt, prior=None):
        assert ld >= width
        self.rows, self.width, self.ld = rows, width, ld
        self.buf = torch.empty((rows + 2 * self.G) * ld, device=DEV, dtype=tdt)
        two = self.buf.element_size() == 2
        self.sent = 0x5A5A if two else 0x5A5A5A5A
        self.ibuf = self.buf.view(torch.int16 if two else torch.int32).view(rows + 2 * self.G, ld)
        self.ibuf.fill_(self.sent)
        self.body = self.buf.view(rows + 2 * self.G, ld)[self.G:self.G + rows]
        if prior is None:
            self.body[:, :width] = float("nan")
        else:
            self.body[:, :width] = prior
        self.ptr = self.body.data_ptr()

    def got(self):
        return self.body[:, :self.width]

    def check(self, what, written=True):
        G, rows = self.G, self.rows
        assert bool((self.ibuf[:G] == self.sent).all()), f"{what}: guard rows BEFORE the output were written"
        assert bool((self.ibuf[G + rows:] == self.sent).all()), f"{what}: guard rows AFTER the output were written"
        assert bool((self.ibuf[G:G + rows, self.width:] == self.sent).all()), \
            f"{what}: columns {self.width}..{self.ld} of the output rows were written"
        if written:
            assert not bool(torch.isnan(self.got().float()).any()), f"{what}: output not fully written"


def attn_reference(q, k, v, dout):
    """fp32 eager attention + autograd on (B,H,N,dh) tensors: O, lse, dQ, dK, dV."""
    q, k, v = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5
    o = torch.softmax(s, dim=-1) @ v
    o.backward(dout.float())
    return o.detach(), torch.logsumexp(s, dim=-1).detach(), q.grad, k.grad, v.grad


def launch_attention(lib, dtype, layout, q, k, v, dout, exact_extent=False):
    """q, k, v, dout: [B, H, N, dh] in the operand dtype (any device).  layout "token": one token-major [B*N, ld] matrix
    (ld = 3D + 8 with NaN in the slack, or exactly 3D with `exact_extent`: then the matrix sits between two NaN blocks of
    one allocation, so any read past its extent poisons the result); "head": zero-padded [B, H, N, DP] matrices.
    The backward consumes the forward's own output.  Returns the two status codes and the `Guarded` out [B*N, D],
    lse [1, B*H*N] and dqkv [B*N, 3D], unchecked."""
    tdt = tdt_of(dtype)
    q, k, v, dout = (t.to(DEV) for t in (q, k, v, dout))
    B, H, N, dh = q.shape
    DP, D = rup(dh, 16), H * dh
    if layout == "token":
        ld = 3 * D if exact_extent else 3 * D + 8
        rows = B * N
        pad = 64 if exact_extent else 0
        store = torch.full(((rows + 2 * pad), ld), float("nan"), device=DEV, dtype=tdt)
        tok = store[pad:pad + rows]
        tok[:, :3 * D] = torch.stack((q, k, v)).permute(1, 3, 0, 2, 4).reshape(rows, 3 * D)
        ptrs = [tok.data_ptr() + j * D * tok.element_size() for j in range(3)]
    else:
        ld = 0
        qkv = torch.zeros(3, B, H, N, DP, device=DEV, dtype=tdt)
        qkv[..., :dh] = torch.stack((q, k, v))
        ptrs = [qkv[j].data_ptr() for j in range(3)]
    dout_tok = dout.permute(0, 2, 1, 3).reshape(B * N, D).contiguous()
    out = Guarded(B * N, D, D, tdt)
    lse = Guarded(1, B * H * N, B * H * N, torch.float32)
    st_f = lib.sgl_op_attn_fwd(dtype, ptrs[0], ptrs[1], ptrs[2], out.ptr, lse.ptr, B, H, N, dh, DP, ld, stream())
    dqkv = Guarded(B * N, 3 * D, 3 * D, tdt)
    delta = torch.empty(2, B, H, N, device=DEV)
    st_b = lib.sgl_op_attn_bwd(dtype, ptrs[0], ptrs[1], ptrs[2], out.ptr, P(dout_tok), lse.ptr, dqkv.ptr, P(delta), B, H, N,
                               dh, DP, ld, stream())
    torch.cuda.synchronize()          # the inputs are released on return
    return st_f, st_b, out, lse, dqkv


def run_attention(lib, dtype, layout, q, k, v, dout, exact_extent=False, written=True):
    """launch_attention with both calls accepted and every guard band checked.  Returns O, lse, dQ, dK, dV as
    [B, H, N, dh] (lse [B, H, N]).  written=False (inputs that hold a NaN on purpose) leaves out the check that no NaN of
    the pre-filled bodies survived; the guard bands are checked all the same."""
    B, H, N, dh = q.shape
    st_f, st_b, out, lse, dqkv = launch_attention(lib, dtype, layout, q, k, v, dout, exact_extent)
    ok(st_f)
    ok(st_b)
    out.check("attention forward out", written)
    lse.check("attention forward lse", written)
    dqkv.check("attention backward dqkv", written)
    O = out.got().view(B, N, H, dh).permute(0, 2, 1, 3)
    g = dqkv.got().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    return O, lse.got().view(B, H, N), g[0], g[1], g[2]


def check_attention(lib, dtype, layout, kind, B, H, N, dh, seed=0, jump_key=None, exact_extent=False):
    tdt = tdt_of(dtype)
    q, k, v, do = kr.attn_inputs(kind, B, H, N, dh, tdt, seed=seed, jump_key=jump_key)
    O, lse, dQ, dK, dV = run_attention(lib, dtype, layout, q, k, v, do, exact_extent)
    r = kr.attn_ref(q.to(DEV), k.to(DEV), v.to(DEV), do.to(DEV))
    fp32_mode = dtype in (F32, BF16X3)
    u = kr.UNIT[tdt]
    what = f"attention {kr.DT_NAME[dtype]} {layout} {kind} B={B} H={H} N={N} dh={dh}"
    bO, bl = kr.attn_fwd_bound(r, u, fp32_mode)
    kr.assert_within(O, r["O"], bO, what + " O")
    kr.assert_within(lse, r["lse"], bl, what + " lse")
    bQ, bK, bV = kr.attn_bwd_bound(r, u, fp32_mode=fp32_mode, tiny=kr.TINY[tdt])
    kr.assert_within(dV, r["dV"], bV, what + " dV")
    kr.assert_within(dK, r["dK"], bK, what + " dK")
    kr.assert_within(dQ, r["dQ"], bQ, what + " dQ")
    return r, (O, dV)
