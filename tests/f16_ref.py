"""CPU reference of the one-product fp16 arithmetic (eval math 'f16'): what the ``*_f16`` kernels compute up to fp32
summation order.  Operands are rounded ONCE by ``round_f16`` (clamp to +-65504, then round to nearest even to fp16), a
product is the single product of the rounded operands (exact in fp32: 11 + 11 significant bits) and products are
accumulated in fp64.  For 3x3 stride-1 pad-1 convolutions the operands that are rounded are the transformed ones of Winograd
F(2x2, 3x3), V = B^T d B and U = G g G^T, formed in fp32 in the operation order of the kernels (tests/x3_ref.py: wino_u, wino_v).
``round_tf32`` is the yardstick of the network tests: the same structure with operands rounded to TF32's 10 explicit mantissa
bits (round half up on the magnitude), the reference's default GPU convolution arithmetic."""
import torch

from tests.x3_ref import Routed, wino_u, wino_v

F16_MAX = 65504.0


def round_f16(x: torch.Tensor) -> torch.Tensor:
    """clamp(+-65504), then round to nearest even to fp16; fp32 tensor holding fp16 values."""
    return x.float().clamp(-F16_MAX, F16_MAX).to(torch.float16).float()


def round_tf32(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> 10 explicit mantissa bits, round half up on the magnitude (add half an ulp to the bit pattern, mask)."""
    b = x.float().contiguous().view(torch.int32)
    return ((b + 0x1000) & ~0x1fff).view(torch.float32)


def one_product_einsum(eq: str, a: torch.Tensor, b: torch.Tensor, rnd=round_f16) -> torch.Tensor:
    """einsum(eq, a, b) on operands rounded once by ``rnd``, fp64 result."""
    return torch.einsum(eq, rnd(a).double(), rnd(b).double())


def f16_matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [m][k] @ b[n][k]^T in one-product fp16 arithmetic, fp64 result [m][n]."""
    return one_product_einsum("mk,nk->mn", a, b)


def one_product_conv3x3(x: torch.Tensor, w: torch.Tensor, rnd=round_f16) -> torch.Tensor:
    """3x3 stride-1 pad-1 convolution of NCHW ``x`` (even H, W) with OIHW ``w`` in one-product Winograd arithmetic; fp64 NCHW
    result without bias."""
    b, c, h, wd = x.shape
    assert h % 2 == 0 and wd % 2 == 0 and tuple(w.shape[1:]) == (c, 3, 3)
    u, v = wino_u(w), wino_v(x)
    m = one_product_einsum("ptc,poc->pto", v.reshape(16, -1, c), u, rnd)        # [16][tiles][cout], fp64
    m = m.reshape(4, 4, b, h // 2, wd // 2, -1)
    s = [[(m[i, 0] + m[i, 1]) + m[i, 2], (m[i, 1] - m[i, 2]) - m[i, 3]] for i in range(4)]
    y = torch.empty((b, h // 2, 2, wd // 2, 2, m.shape[-1]), dtype=torch.float64)
    for xb in range(2):
        y[:, :, 0, :, xb] = (s[0][xb] + s[1][xb]) + s[2][xb]
        y[:, :, 1, :, xb] = (s[1][xb] - s[2][xb]) - s[3][xb]
    return y.reshape(b, h, wd, -1).permute(0, 3, 1, 2).contiguous()


def f16_conv3x3(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return one_product_conv3x3(x, w, round_f16)


def one_product_conv2d(x, w, bias=None, stride=1, padding=0, rnd=round_f16):
    """``F.conv2d`` for the convolutions of the NCSN++ oracle with every contraction in one-product arithmetic: 3x3 stride-1
    pad-1 in Winograd form, everything else as an im2col product.  fp32 result (rounded once from fp64)."""
    co, ci, kh, kw = w.shape
    if (kh, kw, stride, padding) == (3, 3, 1, 1) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0:
        y = one_product_conv3x3(x, w, rnd)
    else:
        b = x.shape[0]
        oh = (x.shape[2] + 2 * padding - kh) // stride + 1
        ow = (x.shape[3] + 2 * padding - kw) // stride + 1
        cols = torch.nn.functional.unfold(x.float(), (kh, kw), padding=padding, stride=stride)      # [B][ci*kh*kw][L]
        y = one_product_einsum("bkl,ok->bol", cols, w.float().reshape(co, -1), rnd).reshape(b, co, oh, ow)
    if bias is not None:
        y = y + bias.double()[None, :, None, None]
    return y.float()


def f16_conv2d(x, w, bias=None, stride=1, padding=0):
    return one_product_conv2d(x, w, bias, stride, padding, round_f16)


def route_oracle(monkeypatch, oracle, rnd=round_f16):
    """tests/x3_ref.py's routing of the oracle (F.conv2d of the network, torch.einsum; not the one-channel FIR filter) with the
    limb product replaced by one product of operands rounded by ``rnd``."""
    import torch.nn.functional as F

    def conv2d(x, w, bias=None, stride=1, padding=0, **kw):
        if kw or w.shape[0] == 1 and w.shape[1] == 1:      # upfirdn2d's filter
            return F.conv2d(x, w, bias, stride, padding, **kw)
        return one_product_conv2d(x, w, bias, stride, padding, rnd)

    def einsum(eq, a, b):
        return one_product_einsum(eq, a, b, rnd).float()
    monkeypatch.setattr(oracle, "F", Routed(F, conv2d=conv2d))
    monkeypatch.setattr(oracle, "torch", Routed(torch, einsum=einsum))
