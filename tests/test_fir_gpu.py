"""Every launch form of the FIR resampler (psld_upfirdn2d_f32, resample.hip) against an fp64 reference.

The host entry point picks one of three NHWC kernels from the taps, the factors and batch * out_h: the 2 x 2-outputs-per-
thread x2-up kernel (four pad-parity instantiations), the one-output x2-down kernel and the generic one (also the fallback
from batch * out_h = 65536 on).  The cases below reach each of them with a 4 x 4 kernel that is neither symmetric nor
separable, with unequal x / y pads, crops, odd output sizes, channel-quad counts that do not divide the 256-thread block,
several blocks in x and ``accumulate``; each NHWC result is checked next to the NCHW kernel on the same data.

Tolerance (derived, element-wise):  |y - ref| <= 18 * 2^-24 * (ref(|x|, |K4|) + |prev|).  An output is a sum of at most 16
products plus the add of ``prev`` under accumulate: the gamma_n bound of a 17-term sum (n u / (1 - n u), u = 2^-24) holds for
every summation order, with or without FMA; 18 u covers it.  The smallest tap (0.1) stands more than 1e4 above the bound, so
a wrong, missing or transposed tap cannot hide in it.  The comparison is <=: an output that only sees padding has bound 0
and must be exactly 0.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psld_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
K4 = np.array([[1, 2, -1, .75], [.5, 3, .25, -1.25], [-2, 1.5, 4, .6], [.1, .2, .3, -.4]], dtype=np.float32)
K4_64 = torch.from_numpy(K4).double()            # the fp32 taps the kernels get, held in fp64
BOUND = 18 * 2.0 ** -24

UP_PADS = [(2, 1, 2, 1), (1, 2, 1, 2), (2, 1, 1, 2), (1, 2, 2, 1), (2, 2, 2, 2), (3, 1, 0, 2), (-1, 3, 2, -1), (1, 1, 1, 1)]
UP_SHAPES = [(2, 4, 5, 7), (3, 40, 9, 6), (1, 132, 3, 3), (2, 8, 1, 1), (1, 260, 2, 3), (1, 132, 3, 20)]
DOWN_PADS = [(1, 1, 1, 1), (2, 1, 1, 2), (0, 2, 2, 0), (2, 2, 1, 1), (-1, 2, 1, 0)]
DOWN_SHAPES = [(2, 4, 10, 14), (3, 40, 9, 7), (1, 132, 6, 6), (2, 8, 4, 4), (1, 260, 5, 8), (1, 132, 6, 40)]


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as _ops
    _ops.lib()
    return _ops


def gen(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ref_upfirdn(x, k, up, down, pads):
    """Zero-insert, pad or crop each side by its own amount (px0, px1, py0, py1), correlate with the flipped kernel,
    decimate - oracle.psld_oracle.upfirdn2d with per-axis pads.  x: [N, C, H, W] fp64."""
    n, c, h, w = x.shape
    kh, kw = k.shape
    px0, px1, py0, py1 = pads
    y = x.reshape(n * c, 1, h, w)
    if up > 1:
        z = y.new_zeros(n * c, 1, h * up, w * up)
        z[:, :, ::up, ::up] = y
        y = z
    y = F.pad(y, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    y = y[:, :, max(-py0, 0): y.shape[2] - max(-py1, 0), max(-px0, 0): y.shape[3] - max(-px1, 0)]
    y = F.conv2d(y, torch.flip(k, [0, 1]).view(1, 1, kh, kw))
    y = y[:, :, ::down, ::down]
    return y.reshape(n, c, y.shape[2], y.shape[3])


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def out_size(h, w, up, down, pads):
    px0, px1, py0, py1 = pads
    sh, sw = h * up + py0 + py1 - 4, w * up + px0 + px1 - 4
    return (sh // down + 1 if sh >= 0 else 0, sw // down + 1 if sw >= 0 else 0)


def ratio(y, ref, bound):
    """Worst |y - ref| / bound over the tensor; where the bound is 0 (an output of padding only) y must be exactly 0."""
    y = y.double().cpu()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert bool(torch.isfinite(y).all()), "an output element was not written"
    err = (y - ref).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "an output that sees only padding is not exactly 0"
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def refused_as_empty(ops, x, up, down, pads, layout):
    """The call names the empty output and writes nothing (a real buffer stands in for the empty one, whose null pointer
    would be refused first)."""
    out = torch.full((64,), NAN, device=DEV)
    with pytest.raises(RuntimeError, match="empty output"):
        ops.upfirdn2d_raw(x, K4, up, down, pads, layout, out=out)
    assert bool(torch.isnan(out).all())


def forward_case(ops, x, up, down, pads, accumulate=False, seed=0):
    """(ratio NHWC, ratio NCHW) of one forward call on x [N, C, H, W] fp32; the output buffers start as NaN, or as a random
    ``prev`` under accumulate."""
    b, c, h, w = x.shape
    oh, ow = out_size(h, w, up, down, pads)
    ref = ref_upfirdn(x.double(), K4_64, up, down, pads)
    bound = ref_upfirdn(x.double().abs(), K4_64.abs(), up, down, pads)
    assert ref.shape == (b, c, oh, ow)
    if pads[0] == pads[2] and pads[1] == pads[3]:
        assert torch.equal(ref, O.upfirdn2d(x.double(), K4_64, up, down, (pads[0], pads[1])))
    prev = gen(b, c, oh, ow, seed=seed + 1) if accumulate else torch.full((b, c, oh, ow), NAN)
    if accumulate:
        ref, bound = ref + prev.double(), bound + prev.double().abs()
    bound = bound * BOUND
    y1 = ops.upfirdn2d_raw(nhwc(x).to(DEV), K4, up, down, pads, 1, out=nhwc(prev).to(DEV), accumulate=accumulate)
    y0 = ops.upfirdn2d_raw(x.to(DEV), K4, up, down, pads, 0, out=prev.to(DEV), accumulate=accumulate)
    return ratio(nchw(y1), ref, bound), ratio(y0, ref, bound)


def test_reference_is_the_oracle_on_symmetric_pads():
    """Host only: the per-axis reference equals oracle.psld_oracle.upfirdn2d bit for bit wherever x and y pads agree,
    and an fp32 evaluation of it stays inside the bound it sets for the kernels (measured: at most 0.17 of it)."""
    x = gen(2, 4, 5, 7, seed=11)
    worst = 0.0
    for up, down, p in [(2, 1, (2, 1)), (2, 1, (1, 2)), (2, 1, (2, 2)), (2, 1, (-1, 3)), (1, 2, (1, 1)), (1, 2, (2, 1)),
                        (1, 1, (2, 1)), (3, 2, (2, 1))]:
        pads = (p[0], p[1], p[0], p[1])
        ref = ref_upfirdn(x.double(), K4_64, up, down, pads)
        assert torch.equal(ref, O.upfirdn2d(x.double(), K4_64, up, down, p))
        bound = ref_upfirdn(x.double().abs(), K4_64.abs(), up, down, pads) * BOUND
        worst = max(worst, ratio(ref_upfirdn(x, K4_64.float(), up, down, pads), ref, bound))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("pads", UP_PADS, ids=lambda p: "pad%d_%d_%d_%d" % p)
def test_up2_quad_kernel(ops, pads):
    """x2 up with the 4 x 4 kernel: upfirdn4_up2_quad_kernel<PY, PX>, PY / PX = parity of the leading y / x pad."""
    worst = [0.0, 0.0]
    for i, (b, c, h, w) in enumerate(UP_SHAPES):
        x = gen(b, c, h, w, seed=100 + i)
        if 0 in out_size(h, w, 2, 1, pads):
            refused_as_empty(ops, nhwc(x).to(DEV), 2, 1, pads, 1)
            continue
        r = forward_case(ops, x, 2, 1, pads)
        worst = [max(a, v) for a, v in zip(worst, r)]
    print(f"FIR up2 quad<{pads[2] & 1},{pads[0] & 1}> pads {pads}: worst error / bound {worst[0]:.3f} (NHWC), {worst[1]:.3f} (NCHW)")
    assert max(worst) <= 1.0, worst


def test_an_empty_output_is_refused(ops):
    """(2, 8, 1, 1) under the crop pads has no output rows: the call is refused, and so is a padded extent one short of the
    kernel under x2 down, which C division would round up to one row."""
    assert 0 in out_size(1, 1, 2, 1, (-1, 3, 2, -1)) and 0 in out_size(1, 1, 1, 2, (1, 1, 1, 1))
    refused_as_empty(ops, torch.zeros(2, 1, 1, 8, device=DEV), 2, 1, (-1, 3, 2, -1), 1)
    refused_as_empty(ops, torch.zeros(2, 1, 1, 8, device=DEV), 1, 2, (1, 1, 1, 1), 1)
    refused_as_empty(ops, torch.zeros(2, 8, 1, 1, device=DEV), 1, 2, (1, 1, 1, 1), 0)


@pytest.mark.parametrize("pads", DOWN_PADS, ids=lambda p: "pad%d_%d_%d_%d" % p)
def test_down2_kernel(ops, pads):
    """x2 down with the 4 x 4 kernel: upfirdn4_nhwc_kernel<1, 2>, all sixteen taps per output."""
    worst = [0.0, 0.0]
    for i, (b, c, h, w) in enumerate(DOWN_SHAPES):
        assert 0 not in out_size(h, w, 1, 2, pads)
        r = forward_case(ops, gen(b, c, h, w, seed=200 + i), 1, 2, pads)
        worst = [max(a, v) for a, v in zip(worst, r)]
    print(f"FIR down2 <1,2> pads {pads}: worst error / bound {worst[0]:.3f} (NHWC), {worst[1]:.3f} (NCHW)")
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("up,down", [(1, 1), (3, 2)])
def test_generic_kernel_with_the_4x4_taps(ops, up, down):
    worst = [0.0, 0.0]
    for i, (b, c, h, w) in enumerate([(2, 4, 5, 7), (3, 40, 9, 6), (1, 132, 3, 20)]):
        r = forward_case(ops, gen(b, c, h, w, seed=300 + i), up, down, (2, 1, 1, 2))
        worst = [max(a, v) for a, v in zip(worst, r)]
    print(f"FIR generic up{up} down{down}: worst error / bound {worst[0]:.3f} (NHWC), {worst[1]:.3f} (NCHW)")
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("up,down,pads,shape", [
    (2, 1, (2, 1, 2, 1), (3, 40, 9, 6)), (2, 1, (1, 2, 1, 2), (3, 40, 9, 6)), (2, 1, (2, 2, 2, 2), (1, 132, 3, 3)),
    (2, 1, (1, 1, 1, 1), (1, 132, 3, 3)), (2, 1, (-1, 3, 2, -1), (2, 4, 5, 7)),
    (1, 2, (1, 1, 1, 1), (3, 40, 9, 7)), (1, 2, (2, 1, 1, 2), (1, 132, 6, 6)),
    (3, 2, (2, 1, 1, 2), (2, 4, 5, 7))])
def test_accumulate(ops, up, down, pads, shape):
    """y += FIR(x) over a random previous content (the backward tape's form), on every NHWC form and the NCHW kernel."""
    r = forward_case(ops, gen(*shape, seed=400), up, down, pads, accumulate=True, seed=401)
    print(f"FIR accumulate up{up} down{down} pads {pads}: error / bound {r[0]:.3f} (NHWC), {r[1]:.3f} (NCHW)")
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("up,down,h,w", [(2, 1, 16, 1), (1, 2, 64, 2)])
def test_the_65536_row_threshold(ops, up, down, h, w):
    """batch * out_h = 2047 * 32 takes the fast form, 2048 * 32 = 65536 the generic kernel: both against fp64."""
    pads = (2, 1, 2, 1) if up == 2 else (1, 1, 1, 1)
    assert out_size(h, w, up, down, pads)[0] == 32
    x = gen(2048, 4, h, w, seed=500)
    ref = ref_upfirdn(x.double(), K4_64, up, down, pads)
    bound = ref_upfirdn(x.double().abs(), K4_64.abs(), up, down, pads) * BOUND
    xd = nhwc(x).to(DEV)
    for b in (2047, 2048):
        out = torch.full((b,) + tuple(ref.shape[2:]) + (4,), NAN, device=DEV)
        y = ops.upfirdn2d_raw(xd[:b], K4, up, down, pads, 1, out=out)
        r = ratio(nchw(y), ref[:b], bound[:b])
        print(f"FIR up{up} down{down} batch {b} ({'fast form' if b * 32 < 65536 else 'generic fallback'}): error / bound {r:.3f}")
        assert r <= 1.0, (b, r)


@pytest.mark.parametrize("in_hw", [(9, 7), (8, 8), (5, 6)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("up,down,pad", [(2, 1, (2, 1)), (1, 2, (1, 1)), (2, 1, (1, 2)), (1, 2, (2, 1))])
def test_backward(ops, up, down, pad, in_hw):
    """ops.upfirdn2d_bwd_raw (the same op with the flipped kernel, up <-> down and the gradient's pads) against fp64 autograd
    of the reference: the gradient of an x2 up lands on the x2-down kernel, that of an x2 down on the quad kernel - with odd
    pad parity for the pads the network does not use.  Bound: the |K4| reference's gradient at |gy|, plus |prev|."""
    b, c = 2, 12
    h, w = in_hw
    pads = (pad[0], pad[1], pad[0], pad[1])
    x = torch.zeros(b, c, h, w, dtype=torch.float64, requires_grad=True)
    y = ref_upfirdn(x, K4_64, up, down, pads)
    gy = gen(*y.shape, seed=600)
    (ref,) = torch.autograd.grad(y, x, gy.double())
    xa = torch.zeros(b, c, h, w, dtype=torch.float64, requires_grad=True)
    (bound,) = torch.autograd.grad(ref_upfirdn(xa, K4_64.abs(), up, down, pads), xa, gy.double().abs())
    prev = gen(b, c, h, w, seed=601)
    worst = 0.0
    for layout in (0, 1):
        for acc in (False, True):
            out = prev.clone() if acc else torch.full((b, c, h, w), NAN)
            out = (nhwc(out) if layout else out).to(DEV)
            dx = ops.upfirdn2d_bwd_raw((nhwc(gy) if layout else gy).to(DEV), K4, up, down, pad, in_hw, layout, out=out,
                                       accumulate=acc)
            assert dx.data_ptr() == out.data_ptr()
            want, bnd = (ref + prev.double(), bound + prev.double().abs()) if acc else (ref, bound)
            worst = max(worst, ratio(nchw(dx) if layout else dx, want, bnd * BOUND))
    print(f"FIR backward of up{up} down{down} pad {pad} at {in_hw}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst
