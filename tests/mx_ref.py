"""Reference MX-fp8 quantizer (OCP MXFP8: e4m3fn elements, one E8M0 scale per 32 K-elements) in float64 torch: the
contract the HIP kernels of the ``mxfp8`` compute mode must meet bit for bit (csrc/mx.hip, include/siglip_hip.h).

Per 32-block of a row with amax = max|x|:
  * e = the smallest integer with amax <= 448 * 2^e, clamped to [-127, 127]; scale byte e + 127;
  * elements x * 2^-e rounded to nearest even into e4m3fn (bias 7, subnormals m * 2^-9 kept, 0x7F = NaN);
  * an all-zero block has scale byte 0 and zero elements; a block holding inf / NaN has scale byte 0xFF and 0x7F elements;
  * K is padded to Kp (a multiple of 128) with zero elements and zero scale bytes.
"""
import torch


def e4m3_decode(codes: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3fn codes -> float64 values (NaN for 0x7F / 0xFF)."""
    b = codes.to(torch.int64)
    e = (b >> 3) & 15
    m = (b & 7).to(torch.float64)
    v = torch.where(e == 0, m / 8.0 * 2.0 ** -6, (1.0 + m / 8.0) * torch.pow(2.0, (e - 7).to(torch.float64)))
    v = torch.where((b & 0x7F) == 0x7F, torch.full_like(v, float("nan")), v)
    return torch.where((b & 0x80) != 0, -v, v)


def scale_exponent(amax: torch.Tensor) -> torch.Tensor:
    """int64 e for float64 amax >= 0 (finite)."""
    m, k = torch.frexp(amax)            # amax = m 2^k, m in [0.5, 1): amax = (2m) 2^(k-1)
    k = k.to(torch.int64) - 1
    e = torch.where(2.0 * m <= 1.75, k - 8, k - 7)
    e = torch.where(amax == 0, torch.full_like(e, -127), e)
    return e.clamp(-127, 127)


def e4m3_encode(y: torch.Tensor) -> torch.Tensor:
    """float64 |y| <= 448 -> uint8 e4m3fn codes, round to nearest even (torch.round is half-to-even)."""
    a = y.abs()
    sign = torch.signbit(y).to(torch.int64) << 7
    sub = torch.round(a * 512.0).to(torch.int64)                         # subnormal grid (8 -> 0x08, the smallest normal)
    f, E = torch.frexp(torch.where(a > 0, a, torch.ones_like(a)))        # a = f 2^E, f in [0.5, 1)
    E = E.to(torch.int64) - 1                                            # a = (2f) 2^E
    q = torch.round((2.0 * f - 1.0) * 8.0).to(torch.int64)               # 3 mantissa bits; 8 carries into the exponent
    normal = ((E + 7) << 3) + q
    code = torch.where(a < 2.0 ** -6, sub, normal)
    return (sign | code).to(torch.uint8)


def quantize(x: torch.Tensor, Kp: int = None):
    """x [M][K] (fp32 / bf16 / fp64 values) -> (codes uint8 [M][Kp], scale bytes uint8 [M][Kp/32])."""
    x = x.detach().to(torch.float64)
    M, K = x.shape
    if Kp is None:
        Kp = (K + 127) // 128 * 128
    xp = torch.zeros(M, Kp, dtype=torch.float64, device=x.device)
    xp[:, :K] = x
    blk = xp.reshape(M, Kp // 32, 32)
    bad = ~torch.isfinite(blk).all(-1)
    amax = torch.where(bad, torch.zeros(M, Kp // 32, dtype=torch.float64, device=x.device),
                       blk.abs().amax(-1))
    e = scale_exponent(amax)
    y = torch.ldexp(torch.where(torch.isfinite(blk), blk, torch.zeros_like(blk)), (-e).unsqueeze(-1).to(torch.float64))
    codes = e4m3_encode(y)
    codes = torch.where(bad.unsqueeze(-1), torch.full_like(codes, 0x7F), codes)
    sc = torch.where(bad, torch.full_like(e, 255), e + 127).to(torch.uint8)
    return codes.reshape(M, Kp), sc


def dequantize(codes: torch.Tensor, sc: torch.Tensor) -> torch.Tensor:
    """(codes [M][Kp], scales [M][Kp/32]) -> float64 [M][Kp]; scale byte 0xFF -> NaN."""
    M, Kp = codes.shape
    s = sc.to(torch.float64)
    mult = torch.where(sc == 255, torch.full_like(s, float("nan")), torch.pow(2.0, s - 127.0))
    return (e4m3_decode(codes).reshape(M, Kp // 32, 32) * mult.unsqueeze(-1)).reshape(M, Kp)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """x [..., K] -> the float64 values its MX-fp8 quantization represents (same shape)."""
    K = x.shape[-1]
    q, s = quantize(x.reshape(-1, K))
    return dequantize(q, s)[:, :K].reshape(x.shape)
