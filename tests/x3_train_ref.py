"""CPU reference of the two-limb arithmetic of a recording pass (record math 'bf16x3'): the data gradient and the
Winograd-domain weight gradient of a 3x3 stride-1 pad-1 convolution, on top of tests/x3_ref.py.

Weight gradient (csrc/wgrad_wino.hip): M = A dY A^T of every 2x2 tile of the output gradient and V = B^T d B of the 4x4 input
tile are formed in fp32 - columns first, then rows, as the kernel's producers do -, split by ``split2``, multiplied over the
tiles as hi*lo + lo*hi + hi*hi per position (fp64 accumulation here, fp32 in the kernel), and dg = G^T dU G.
Data gradient: the forward convolution on the transposed weights rotated by 180 degrees (csrc/conv_wino.hip, dgrad = 1)."""
import torch
import torch.nn.functional as F

from tests import x3_ref as X

_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


def _a_combo(y0, y1):
    """Rows of A = [[1, 0], [1, 1], [1, -1], [0, -1]] applied to a pair."""
    return [y0, y0 + y1, y0 - y1, -y1]


def _bt_combo(d0, d1, d2, d3):
    """Rows of B^T applied to four values."""
    return [d0 - d2, d1 + d2, d2 - d1, d1 - d3]


def wino_m(dy: torch.Tensor) -> torch.Tensor:
    """M = A dY A^T of the 2x2 tiles of an NCHW output gradient, fp32, [16][B][H/2][W/2][C] (position = 4 * row + column)."""
    b, c, h, w = dy.shape
    t = dy.float().reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5)       # [B][H/2][W/2][C][2][2]
    cols = [_a_combo(t[..., r, 0], t[..., r, 1]) for r in range(2)]                     # [row][4 column combos]
    return torch.stack([e for i in range(4) for e in [_a_combo(cols[0][j], cols[1][j])[i] for j in range(4)]], 0)


def wino_v_cols_first(x: torch.Tensor) -> torch.Tensor:
    """V = B^T d B of the 4x4 input tiles (stride 2) of the zero-padded NCHW input, fp32, [16][B][H/2][W/2][C]; the column
    combination is formed first (x3_ref.wino_v, the forward kernel's order, forms the row combination first)."""
    xp = F.pad(x.float(), (1, 1, 1, 1))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2).permute(0, 2, 3, 1, 4, 5)                    # [B][H/2][W/2][C][4][4]
    cols = [_bt_combo(d[..., r, 0], d[..., r, 1], d[..., r, 2], d[..., r, 3]) for r in range(4)]
    return torch.stack([e for i in range(4) for e in
                        [_bt_combo(cols[0][j], cols[1][j], cols[2][j], cols[3][j])[i] for j in range(4)]], 0)


def two_limb_wgrad3x3(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Weight gradient [cout][cin][3][3] (fp64) of the 3x3 stride-1 pad-1 convolution y = conv(x, w) from NCHW ``x`` and
    ``dy`` (even H, W) in two-limb Winograd-domain arithmetic."""
    cin, cout = x.shape[1], dy.shape[1]
    m, v = wino_m(dy).reshape(16, -1, cout), wino_v_cols_first(x).reshape(16, -1, cin)
    du = X.two_limb_einsum("pto,ptc->poc", m, v).reshape(4, 4, cout, cin)               # fp64
    return torch.einsum("ia,jb,ijoc->ocab", _G, _G, du)


def two_limb_dgrad3x3(dy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Data gradient (fp64, NCHW) of the same convolution: ``two_limb_conv3x3`` on rotated, transposed weights."""
    return X.two_limb_conv3x3(dy, w.flip(2, 3).transpose(0, 1).contiguous())


class _Conv3x3(torch.autograd.Function):
    """3x3 stride-1 pad-1 convolution whose forward, data gradient and weight gradient are the two-limb ones."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return X.two_limb_conv3x3(x, w).float()

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return two_limb_dgrad3x3(dy, w).float(), two_limb_wgrad3x3(x, dy).float()


class _Matmul(torch.autograd.Function):
    """einsum(eq, a, b) of two operands with the contraction of all three passes in two-limb arithmetic (the pointwise and
    NIN weight gradients stay three-limb on the GPU; two limbs here bound the error from above)."""

    @staticmethod
    def forward(ctx, eq, a, b):
        ctx.eq = eq
        ctx.save_for_backward(a, b)
        return X.two_limb_einsum(eq, a, b).float()

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ia, rest = ctx.eq.split(",")
        ib, io = rest.split("->")
        return None, X.two_limb_einsum(f"{io},{ib}->{ia}", g, b).float(), X.two_limb_einsum(f"{ia},{io}->{ib}", a, g).float()


def two_limb_conv2d_autograd(x, w, bias=None, stride=1, padding=0):
    """``F.conv2d`` of the oracle's network with every contraction of forward AND backward in two-limb arithmetic."""
    co, ci, kh, kw = w.shape
    if (kh, kw, stride, padding) == (3, 3, 1, 1) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0:
        y = _Conv3x3.apply(x, w)
    else:
        b = x.shape[0]
        oh = (x.shape[2] + 2 * padding - kh) // stride + 1
        ow = (x.shape[3] + 2 * padding - kw) // stride + 1
        cols = F.unfold(x, (kh, kw), padding=padding, stride=stride)                    # [B][ci*kh*kw][L]
        y = _Matmul.apply("bkl,ok->bol", cols, w.reshape(co, -1)).reshape(b, co, oh, ow)
    if bias is not None:
        y = y + bias[None, :, None, None]
    return y


def route_oracle_autograd(monkeypatch, oracle):
    """x3_ref.route_oracle for a pass that is differentiated: the oracle's convolutions and einsums through the two-limb
    forward, data gradient and weight gradient."""
    def conv2d(x, w, bias=None, stride=1, padding=0, **kw):
        if kw or w.shape[0] == 1 and w.shape[1] == 1:      # upfirdn2d's filter
            return F.conv2d(x, w, bias, stride, padding, **kw)
        return two_limb_conv2d_autograd(x, w, bias, stride, padding)

    def einsum(eq, a, b):
        return _Matmul.apply(eq, a, b)
    monkeypatch.setattr(oracle, "F", X.Routed(F, conv2d=conv2d))
    monkeypatch.setattr(oracle, "torch", X.Routed(torch, einsum=einsum))
