"""CPU reference of record f16 (``--train-math f16``): the arithmetic of a recording pass whose forward and data-gradient
launches run on ONE fp16 product, on top of tests/f16_ref.py and tests/x3_train_ref.py.

Forward: f16_ref's one-product convolution and einsum.
Data gradient: the weight-side operand is rounded once to fp16; the activation-side operand - the incoming gradient dy, for a 3x3
stride-1 pad-1 convolution its Winograd transform V = B^T dy B formed in fp32 - is multiplied by 2^shift, clamped to +-65504 and
rounded once to fp16; products are accumulated in fp64 and the result is multiplied by 2^-shift.  Both factors are powers of
two: the rounding is the only error, and the shift only decides WHERE in fp16's range it happens (gradients of a mean-reduced
loss are ~2/N: without a shift they sit among fp16's subnormals, spacing 2^-24, or round to zero).
Weight gradient: x3_train_ref's two-limb one (the GPU keeps every weight gradient on limbs).
"""
import torch
import torch.nn.functional as F

from tests import x3_ref as X
from tests import x3_train_ref as XT
from tests.f16_ref import F16_MAX, one_product_conv2d, one_product_einsum, round_f16

GRAD_SHIFT_MAX = 24


def shift_for(divisor: int) -> int:
    """The shift rule of the mode: min(24, ceil(log2 N)) of the loss's divisor N (0 for N <= 1)."""
    return min(GRAD_SHIFT_MAX, (int(divisor) - 1).bit_length()) if divisor > 1 else 0


def round_f16_shifted(x: torch.Tensor, shift: int) -> torch.Tensor:
    """round_f16(x * 2^shift): the activation-side operand of a data-gradient launch (fp32 tensor holding fp16 values)."""
    return round_f16(x.float() * float(2.0 ** shift))


def _census(census, x: torch.Tensor, shift: int):
    """One site's row of the range census: what the rounding of x * 2^shift meets."""
    if census is None:
        return
    a = (x.float() * float(2.0 ** shift)).abs()
    nz = a > 0
    census.append({"max": float(a.max()), "nonzero": int(nz.sum()), "below_2m14": int((nz & (a < 2.0 ** -14)).sum()),
                   "below_2m25": int((nz & (a < 2.0 ** -25)).sum()), "clamped": int((a > F16_MAX).sum()),
                   "median": float(a[nz].median()) if bool(nz.any()) else 0.0})


def f16s_einsum(eq: str, g: torch.Tensor, w: torch.Tensor, shift: int, census=None) -> torch.Tensor:
    """einsum(eq, g, w) with g (activation side) shifted and rounded once, w rounded once; fp64 result, shift undone."""
    _census(census, g, shift)
    return torch.einsum(eq, round_f16_shifted(g, shift).double(), round_f16(w).double()) * float(2.0 ** -shift)


def f16s_conv3x3(x: torch.Tensor, w: torch.Tensor, shift: int, census=None) -> torch.Tensor:
    """f16_ref.one_product_conv3x3 with the operand shift on V: 3x3 stride-1 pad-1 convolution of NCHW ``x`` with OIHW ``w``,
    fp64 NCHW result.  shift = 0 is f16_ref.f16_conv3x3."""
    b, c, h, wd = x.shape
    assert h % 2 == 0 and wd % 2 == 0 and tuple(w.shape[1:]) == (c, 3, 3)
    u, v = X.wino_u(w), X.wino_v(x)
    m = f16s_einsum("ptc,poc->pto", v.reshape(16, -1, c), u, shift, census)        # [16][tiles][cout], fp64
    m = m.reshape(4, 4, b, h // 2, wd // 2, -1)
    s = [[(m[i, 0] + m[i, 1]) + m[i, 2], (m[i, 1] - m[i, 2]) - m[i, 3]] for i in range(4)]
    y = torch.empty((b, h // 2, 2, wd // 2, 2, m.shape[-1]), dtype=torch.float64)
    for xb in range(2):
        y[:, :, 0, :, xb] = (s[0][xb] + s[1][xb]) + s[2][xb]
        y[:, :, 1, :, xb] = (s[1][xb] - s[2][xb]) - s[3][xb]
    return y.reshape(b, h, wd, -1).permute(0, 3, 1, 2).contiguous()


def f16s_dgrad3x3(dy: torch.Tensor, w: torch.Tensor, shift: int, census=None) -> torch.Tensor:
    """Data gradient (fp64, NCHW) of y = conv3x3(x, w): the shifted convolution of dy with the transposed, rotated weights."""
    return f16s_conv3x3(dy, w.flip(2, 3).transpose(0, 1).contiguous(), shift, census)


def f16s_matmul_dgrad(dy: torch.Tensor, w: torch.Tensor, shift: int) -> torch.Tensor:
    """dx [m][k] = dy [m][n] @ w [n][k] in the mode's data-gradient arithmetic, fp64."""
    return f16s_einsum("mn,nk->mk", dy, w, shift)


def _ctx_shift(state):
    return state["shift"]


def make_autograd(state):
    """The two autograd functions of a routed oracle; ``state`` = {"shift": int, "census": list or None}."""

    class Conv3x3(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w):
            ctx.save_for_backward(x, w)
            return one_product_conv2d(x, w, None, 1, 1, round_f16)

        @staticmethod
        def backward(ctx, dy):
            x, w = ctx.saved_tensors
            return f16s_dgrad3x3(dy, w, state["shift"], state["census"]).float(), XT.two_limb_wgrad3x3(x, dy).float()

    class Matmul(torch.autograd.Function):
        """einsum(eq, a, b).  An operand that is a parameter (a leaf that requires a gradient) is the weight side: its
        gradient is the two-limb one, the other operand's the shifted fp16 one.  Two activations (the attention products,
        which stay on limbs on the GPU): both gradients in the shifted fp16 arithmetic - a bound from above."""

        @staticmethod
        def forward(ctx, eq, a, b, a_is_w, b_is_w):
            ctx.eq, ctx.a_is_w, ctx.b_is_w = eq, a_is_w, b_is_w
            ctx.save_for_backward(a, b)
            return one_product_einsum(eq, a, b, round_f16).float()

        @staticmethod
        def backward(ctx, g):
            a, b = ctx.saved_tensors
            ia, rest = ctx.eq.split(",")
            ib, io = rest.split("->")
            sh, cen = state["shift"], state["census"]
            if ctx.a_is_w:
                da = X.two_limb_einsum(f"{io},{ib}->{ia}", g, b)
            else:
                da = f16s_einsum(f"{io},{ib}->{ia}", g, b, sh, cen)
            if ctx.b_is_w:
                db = X.two_limb_einsum(f"{ia},{io}->{ib}", a, g)
            else:       # g is the activation-side operand here as well: it goes second in the equation, shifted all the same
                _census(cen, g, sh)
                db = torch.einsum(f"{ia},{io}->{ib}", round_f16(a).double(), round_f16_shifted(g, sh).double()) * float(2.0 ** -sh)
            return None, da.float(), db.float(), None, None

    return Conv3x3, Matmul


def _is_param(t: torch.Tensor) -> bool:
    return bool(t.requires_grad and t.is_leaf)


def route_oracle_autograd(monkeypatch, oracle, shift: int, census=None):
    """x3_train_ref.route_oracle_autograd for record f16: the oracle's convolutions and einsums through the one-product forward,
    the shifted fp16 data gradient and the two-limb weight gradient.  ``census``: a list that receives one row per data-gradient
    site of every backward pass (what the rounding of dy * 2^shift meets).  Returns the state dict (its "shift" may be changed
    between passes)."""
    state = {"shift": int(shift), "census": census}
    Conv3x3, Matmul = make_autograd(state)

    def conv2d(x, w, bias=None, stride=1, padding=0, **kw):
        if kw or w.shape[0] == 1 and w.shape[1] == 1:      # upfirdn2d's filter
            return F.conv2d(x, w, bias, stride, padding, **kw)
        co, ci, kh, kw_ = w.shape
        if (kh, kw_, stride, padding) == (3, 3, 1, 1) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0:
            y = Conv3x3.apply(x, w)
        else:
            b = x.shape[0]
            oh = (x.shape[2] + 2 * padding - kh) // stride + 1
            ow = (x.shape[3] + 2 * padding - kw_) // stride + 1
            cols = F.unfold(x, (kh, kw_), padding=padding, stride=stride)                    # [B][ci*kh*kw][L]
            y = Matmul.apply("bkl,ok->bol", cols, w.reshape(co, -1), False, True).reshape(b, co, oh, ow)
        if bias is not None:
            y = y + bias[None, :, None, None]
        return y

    def einsum(eq, a, b):
        return Matmul.apply(eq, a, b, _is_param(a), _is_param(b))
    monkeypatch.setattr(oracle, "F", X.Routed(F, conv2d=conv2d))
    monkeypatch.setattr(oracle, "torch", X.Routed(torch, einsum=einsum))
    return state
