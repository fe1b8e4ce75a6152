"""CPU reference of the two-limb arithmetic (math mode 'bf16x3'): what the ``*_x3`` kernels compute up to fp32 summation
order.  Operands are split by ``split2`` (hi = rne_bf16(x), lo = rne_bf16(x - hi): limbs 0 and 1 of the three-limb split),
a product is hi*hi + (hi*lo + lo*hi), and the three products are accumulated in fp64.  For 3x3 stride-1 pad-1
convolutions the operands that are split are the transformed ones of Winograd F(2x2, 3x3), V = B^T d B and U = G g G^T,
formed in fp32 in the operation order of the kernels (csrc/conv_wino.hip: wino_pack_item, transform)."""
import torch


def split2(x: torch.Tensor):
    """(hi, lo) as fp32 tensors holding bf16 values."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def split3(x: torch.Tensor):
    """The three-limb split of csrc/limb.h (hi + mid + lo == x), as fp32 tensors holding bf16 values."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    r = x - hi
    mid = r.to(torch.bfloat16).float()
    lo = (r - mid).to(torch.bfloat16).float()
    return hi, mid, lo


def two_limb_einsum(eq: str, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """einsum(eq, a, b) in two-limb arithmetic, fp64 result."""
    (ah, al), (bh, bl) = split2(a), split2(b)
    ah, al, bh, bl = ah.double(), al.double(), bh.double(), bl.double()
    return (torch.einsum(eq, al, bh) + torch.einsum(eq, ah, bl)) + torch.einsum(eq, ah, bh)


def two_limb_matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [m][k] @ b[n][k]^T in two-limb arithmetic, fp64 result [m][n]."""
    return two_limb_einsum("mk,nk->mn", a, b)


def wino_u(w: torch.Tensor) -> torch.Tensor:
    """U = G g G^T of OIHW 3x3 weights, fp32, [16 positions][cout][cin] (position = 4 * row + column)."""
    g = w.float()

    def gmul(g0, g1, g2):
        return [g0, 0.5 * ((g0 + g2) + g1), 0.5 * ((g0 + g2) - g1), g2]
    rows = gmul(g[:, :, 0, :], g[:, :, 1, :], g[:, :, 2, :])            # G g: four rows of [co][ci][3]
    u = [e for r in rows for e in gmul(r[..., 0], r[..., 1], r[..., 2])]
    return torch.stack(u, 0)


def wino_v(x: torch.Tensor) -> torch.Tensor:
    """V = B^T d B of the 4x4 input tiles (stride 2) of the zero-padded NCHW input, fp32, [16][B][H/2][W/2][C]."""
    xp = torch.nn.functional.pad(x.float(), (1, 1, 1, 1))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)          # [B][C][H/2][W/2][4][4]
    d = d.permute(0, 2, 3, 1, 4, 5)

    def bmul(d0, d1, d2, d3):
        return [d0 - d2, d1 + d2, d2 - d1, d1 - d3]
    rows = bmul(d[..., 0, :], d[..., 1, :], d[..., 2, :], d[..., 3, :])
    v = [e for r in rows for e in bmul(r[..., 0], r[..., 1], r[..., 2], r[..., 3])]
    return torch.stack(v, 0)


def two_limb_conv3x3(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """3x3 stride-1 pad-1 convolution of NCHW ``x`` (even H, W) with OIHW ``w`` in two-limb Winograd arithmetic; fp64 NCHW
    result without bias."""
    b, c, h, wd = x.shape
    assert h % 2 == 0 and wd % 2 == 0 and tuple(w.shape[1:]) == (c, 3, 3)
    u, v = wino_u(w), wino_v(x)
    m = two_limb_einsum("ptc,poc->pto", v.reshape(16, -1, c), u)        # [16][tiles][cout], fp64
    m = m.reshape(4, 4, b, h // 2, wd // 2, -1)
    s = [[(m[i, 0] + m[i, 1]) + m[i, 2], (m[i, 1] - m[i, 2]) - m[i, 3]] for i in range(4)]
    y = torch.empty((b, h // 2, 2, wd // 2, 2, m.shape[-1]), dtype=torch.float64)
    for xb in range(2):
        y[:, :, 0, :, xb] = (s[0][xb] + s[1][xb]) + s[2][xb]
        y[:, :, 1, :, xb] = (s[1][xb] - s[2][xb]) - s[3][xb]
    return y.reshape(b, h, wd, -1).permute(0, 3, 1, 2).contiguous()


def two_limb_conv2d(x, w, bias=None, stride=1, padding=0):
    """``F.conv2d`` for the convolutions of the NCSN++ oracle with every contraction in two-limb arithmetic: 3x3 stride-1
    pad-1 in Winograd form, everything else as an im2col product.  fp32 result (rounded once from fp64)."""
    co, ci, kh, kw = w.shape
    if (kh, kw, stride, padding) == (3, 3, 1, 1) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0:
        y = two_limb_conv3x3(x, w)
    else:
        b = x.shape[0]
        oh = (x.shape[2] + 2 * padding - kh) // stride + 1
        ow = (x.shape[3] + 2 * padding - kw) // stride + 1
        cols = torch.nn.functional.unfold(x.float(), (kh, kw), padding=padding, stride=stride)      # [B][ci*kh*kw][L]
        y = two_limb_einsum("bkl,ok->bol", cols, w.float().reshape(co, -1)).reshape(b, co, oh, ow)
    if bias is not None:
        y = y + bias.double()[None, :, None, None]
    return y.float()


class Routed:
    """A stand-in for a module (``torch`` / ``torch.nn.functional``) with some attributes replaced."""

    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getattr__(self, name):
        over = object.__getattribute__(self, "_over")
        return over[name] if name in over else getattr(object.__getattribute__(self, "_base"), name)


def route_oracle(monkeypatch, oracle):
    """Route the oracle's network contractions (F.conv2d of the network, torch.einsum) through the two-limb arithmetic.
    The FIR resampling filter (a one-channel F.conv2d) is not a limb product on the GPU either and stays as it is."""
    import torch.nn.functional as F

    def conv2d(x, w, bias=None, stride=1, padding=0, **kw):
        if kw or w.shape[0] == 1 and w.shape[1] == 1:      # upfirdn2d's filter
            return F.conv2d(x, w, bias, stride, padding, **kw)
        return two_limb_conv2d(x, w, bias, stride, padding)

    def einsum(eq, a, b):
        return two_limb_einsum(eq, a, b).float()
    monkeypatch.setattr(oracle, "F", Routed(F, conv2d=conv2d))
    monkeypatch.setattr(oracle, "torch", Routed(torch, einsum=einsum))
