"""The kv8 cache format restated on the CPU (numpy-free torch): what csrc/paged_attn.hip must write
and read back, bit for bit.  Importing it needs no GPU.

A row -- one position of one kv head, D 16-bit elements of K (after the rotary) or of V -- becomes D OCP
E4M3 codes (torch.float8_e4m3fn) and one scale byte s = e + 127 that stands for 2^e:
  a = the row's largest |x| in fp32;  an inf or NaN anywhere: s = 255, every code 0x7F;
  a = m 2^x, m in [1, 2):  e = x - 8 if m <= 1.75 else x - 7 -- the smallest e with a 2^-e <= 448;
  e = max(e, e_min), e_min = -15 (fp16) / -124 (bf16);  code i = RNE_e4m3(x_i 2^-e).
The scaled magnitude never exceeds 448, so torch's CPU cast to float8_e4m3fn (round to nearest even)
serves as the rounding.  Dequantise: decode(code) 2^e, rounded to nearest even into the storage dtype;
NaN where s = 255 or the code is 0x7F / 0xFF.

Pool layout: uint8 [P, Hkv, 128 (D + 1)]; the block of (page, kv head) is its 128 D codes as [128, D],
then its 128 scale bytes."""
import torch

PAGE = 128
E_MIN = {torch.float16: -15, torch.bfloat16: -124}
E_MAX = {torch.float16: 8, torch.bfloat16: 120}      # the largest e the rule produces
F8 = torch.float8_e4m3fn


def scale_exponent(a: torch.Tensor, dtype) -> torch.Tensor:
    """e (int32) of finite absmax values a (fp32, >= 0), from the exponent and mantissa bits."""
    bits = a.to(torch.float32).contiguous().view(torch.int32)
    e = (bits >> 23) - 127 - 8 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    return e.clamp(min=E_MIN[dtype])


def quantize_rows(x: torch.Tensor):
    """x [..., D] fp16 / bf16 -> (codes uint8 [..., D], scales uint8 [...])."""
    assert x.dtype in E_MIN
    xf = x.detach().cpu().to(torch.float32)
    bad = ~torch.isfinite(xf).all(-1)
    a = torch.where(bad, torch.zeros(()), xf.abs().amax(-1))
    e = scale_exponent(a, x.dtype)
    scaled = (xf.double() * torch.pow(2.0, -e.double()).unsqueeze(-1)).to(torch.float32)   # exact
    scaled = torch.where(bad.unsqueeze(-1), torch.zeros(()), scaled)
    assert float(scaled.abs().max()) <= 448.0 if scaled.numel() else True
    codes = scaled.to(F8).view(torch.uint8).clone()
    codes[bad] = 0x7F
    scales = torch.where(bad, torch.full_like(e, 255), e + 127).to(torch.uint8)
    return codes, scales


def dequantize_rows(codes: torch.Tensor, scales: torch.Tensor, dtype) -> torch.Tensor:
    """codes uint8 [..., D], scales uint8 [...] -> [..., D] of dtype (fp16 / bf16)."""
    codes, scales = codes.cpu(), scales.cpu()
    val = codes.contiguous().view(F8).to(torch.float32).double()
    e = scales.to(torch.int32) - 127
    out = (val * torch.pow(2.0, e.double()).unsqueeze(-1)).to(torch.float32)   # exact: at most 4 significant bits
    nan = (scales == 255).unsqueeze(-1) | ((codes & 0x7F) == 0x7F)
    out = torch.where(nan, torch.full((), float("nan")), out)
    return out.to(dtype)


def pack_pool(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """codes uint8 [P, Hkv, 128, D], scales uint8 [P, Hkv, 128] -> pool uint8 [P, Hkv, 128 (D + 1)]."""
    P, Hkv, page, D = codes.shape
    assert page == PAGE and scales.shape == (P, Hkv, PAGE)
    return torch.cat((codes.reshape(P, Hkv, PAGE * D), scales), -1).contiguous()


def unpack_pool(pool: torch.Tensor, D: int):
    """pool uint8 [P, Hkv, 128 (D + 1)] -> (codes [P, Hkv, 128, D], scales [P, Hkv, 128])."""
    P, Hkv, W = pool.shape
    assert W == PAGE * (D + 1)
    return pool[..., :PAGE * D].reshape(P, Hkv, PAGE, D), pool[..., PAGE * D:]


def quantize_pool(pool16: torch.Tensor) -> torch.Tensor:
    """A 16-bit pool [P, Hkv, 128, D] as the kv8 pool of its rows."""
    return pack_pool(*quantize_rows(pool16))


def dequantize_pool(pool8: torch.Tensor, D: int, dtype) -> torch.Tensor:
    """A kv8 pool as the 16-bit pool [P, Hkv, 128, D] it reads back as."""
    return dequantize_rows(*unpack_pool(pool8.cpu(), D), dtype)
