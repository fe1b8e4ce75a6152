"""Launch geometries and alignment fallbacks of the bandwidth-bound reductions and sweeps, each against an fp64 reference.

Column reductions (psld_colsum_f32, psld_bias_grad_f32, psld_bias_grad_seg_f32): the block is (c / 4 channel quads) x
(256 / (c / 4) pixel lanes) - widths whose quad count does not divide 256 (c = 160 / 320 / 480: 240 threads), one lane
(c >= 516), lanes clipped by hw, a short last chunk, one chunk at batch >= 1024, more than 64 images (and not a multiple of
64) in the per-image / total pass, and the longest fp32 run a thread sums (a 128 x 128 map at c = 128).
Grid-stride sweeps (psld_grad_norm_f32, psld_adam_ema_f32) at sizes where the grid wraps and the fp32 run is flushed to
fp64, and every path a pointer that is not 16-byte aligned takes (grad_norm, axpby, softmax_rows, reduce_slabs, colsum).
Gates are the ones the aligned / narrow cases in test_kernels_gpu.py already use.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psld_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as _ops
    _ops.lib()
    return _ops


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def off1(t):
    """The same values on a device pointer one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------------------------------
# column reductions
# ---------------------------------------------------------------------------------------------------
# (batch, hw, c, ld, column offset)
COLSUM_SHAPES = [(5, 81, 160, 160, 0), (3, 100, 320, 352, 0), (2, 256, 480, 480, 0), (130, 16, 640, 640, 0),
                 (65, 64, 128, 384, 128), (1100, 8, 32, 32, 0), (2, 1024, 1024, 1024, 0), (3, 64, 768, 768, 0),
                 (2, 16384, 128, 128, 0)]


@pytest.mark.parametrize("b,hw,c,ld,col0", COLSUM_SHAPES, ids=lambda v: str(v))
def test_column_reductions(ops, b, hw, c, ld, col0):
    x = gen(b, hw, ld, seed=700 + c + hw).to(DEV)
    sl = x.view(-1)[col0:]
    ref = x[..., col0:col0 + c].double().cpu().sum(dim=1)              # [b][c] per-image sums
    tot = 0.5 * ref.sum(dim=0)
    ldp = c + 8
    per, out = nan(b, ldp), nan(c)
    ops.bias_grad(sl, ld, b, hw, c, out, 0.5, per, ldp)
    e_per, e_tot = rel_l2(per[:, :c], ref), rel_l2(out, tot)
    assert bool(torch.isnan(per[:, c:]).all()), "bias_grad wrote between the rows of per_image"
    out2 = nan(c)
    ops.bias_grad(sl, ld, b, hw, c, out2, 0.5, None)
    e_tot2 = rel_l2(out2, tot)
    cs = nan(b, c)
    ops.colsum(sl, ld, b, hw, c, cs, 0.5)
    e_cs = rel_l2(cs, 0.5 * ref)
    print(f"column sums ({b}, {hw}, {c}, ld {ld}): rel-L2 per-image {e_per:.2e}, total {e_tot:.2e}, "
          f"total without per_image {e_tot2:.2e}, colsum {e_cs:.2e}")
    assert e_per < 1e-6 and e_tot < 1e-6 and e_tot2 < 1e-6 and e_cs < 1e-6
    assert torch.equal(out, out2)
    if c % 12 == 0:
        seg = c // 3
        outs = [nan(seg) for _ in range(3)]
        ops.bias_grad_seg(sl, ld, b, hw, outs, seg, 0.5)
        e_seg = rel_l2(torch.cat(outs), tot)
        print(f"column sums ({b}, {hw}, 3 x {seg}): rel-L2 of the three segments {e_seg:.2e}")
        assert e_seg < 1e-6
        assert torch.equal(torch.cat(outs), out)


@pytest.mark.parametrize("b,hw,c,ld,shift", [(3, 7, 128, 128, 0), (2, 20, 1028, 1028, 0), (3, 50, 64, 70, 0), (3, 300, 128, 128, 1)],
                         ids=["hw7", "c1028", "ld70", "pointer+1"])
def test_colsum_scalar_fallback(ops, b, hw, c, ld, shift):
    x = gen(b * hw * ld, seed=720 + hw)
    xd = off1(x) if shift else x.to(DEV)
    cs = nan(b, c)
    ops.colsum(xd, ld, b, hw, c, cs, 0.5)
    assert rel_l2(cs, 0.5 * x.view(b, hw, ld)[..., :c].double().sum(dim=1)) < 1e-6


def test_bias_grad_refuses_what_its_vector_kernel_cannot_take(ops):
    for b, hw, c, ld in [(2, 20, 1028, 1028), (3, 50, 64, 70)]:
        x = gen(b, hw, ld, seed=730).to(DEV)
        out = nan(c)
        with pytest.raises(RuntimeError, match="psld_bias_grad_f32: needs c"):
            ops.bias_grad(x, ld, b, hw, c, out, 0.5)
        assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------------
# gradient norm, Adam + EMA
# ---------------------------------------------------------------------------------------------------
def test_grad_norm_long_and_unaligned(ops):
    """n = 9 * 2^21 + 100003: every thread of the 2048 x 256 grid takes more than eight float4, so the fp32 run is flushed
    into the fp64 sum; the same buffer from element 1 on takes the scalar loop."""
    n = 9 * 2 ** 21 + 100003
    g = gen(n + 1, seed=740)
    gd = g.to(DEV)
    norm = nan(1, dtype=torch.float64)
    for first in (0, 1):
        v = gd[first:first + n]
        assert v.data_ptr() % 16 == 4 * first
        norm.fill_(NAN)
        ops.grad_norm(v, norm)
        want = g[first:first + n].double().norm().item()
        err = abs(norm.item() - want) / want
        print(f"grad_norm n = {n} {'unaligned' if first else 'aligned'}: relative error {err:.2e}")
        assert err < 1e-5
    for first in (0, 1):
        norm.fill_(NAN)
        ops.grad_norm(gd[first:first + 3], norm)
        want = g[first:first + 3].double().norm().item()
        assert abs(norm.item() - want) < 1e-5 * want


ADAM_N = 2 * 2 ** 20 + 100003       # more than the 4096 x 256 threads of the launch: the grid wraps
LR, B1, B2, EPS, TAU = 2e-4, 0.9, 0.999, 1e-8, 0.9999


@pytest.fixture(scope="module")
def adam_inputs():
    """(p, g, g with the sign of p).  The weight-decay cases take the third: where g + wd p cancels, the normalised step
    lr m / sqrt(v) turns the half ulp between a fused and an unfused g + wd p into an error of lr ulp(wd p) / |g + wd p| in
    p, which no fp32 kernel keeps below the gate on every one of 2.2 M unit-normal elements.  With the independent g of
    these seeds and max_norm = 1 (clip coefficient from the fp64 norm) it is element 864622: p = 0.10113164, clipped
    g = -1.0113097e-3, so g + wd p = 6.75e-9 when the product is rounded before the add (O.adam_step in fp32) and 6.70e-9
    when the sum is rounded once (fp64 sum cast to fp32) - both below eps = 1e-8 - and after two steps the two CPU runs hold
    p = 0.10119615 and 0.10119651, 3.6e-7 apart against a gate of 2e-7 + 5e-7 |p| = 2.5e-7; every other element agrees.
    With equal signs the sum cannot cancel and the gate holds as derived."""
    p, g = gen(ADAM_N, seed=750), gen(ADAM_N, seed=751) * 0.01
    return p, g, g.abs() * torch.sign(p)


def _adam_gpu(ops, p, g, wd, max_norm, with_norm, with_ema, write_g=False, steps=2):
    """Two fused steps; returns the device tensors (p, m, v, ema or None, g) and the norm of every step."""
    pd, gd = p.to(DEV).clone(), g.to(DEV).clone()
    md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
    ed = pd.clone() if with_ema else None
    norm = nan(1, dtype=torch.float64) if with_norm else None
    norms, grads = [], []
    for step in range(1, steps + 1):
        if with_norm:
            ops.grad_norm(gd, norm)
            norms.append(norm.item())
        ops.adam_ema(pd, gd, md, vd, ed, norm, max_norm, LR, B1, B2, EPS, wd, step, TAU, write_clipped_grad=write_g)
        if write_g:
            grads.append(gd.cpu())
    return pd, md, vd, ed, grads, norms


def _adam_ref(p, g, wd, max_norm, steps=2, carry_clipped=False):
    """The oracle's clip, Adam step and EMA.  The clip coefficient comes from the fp64 norm: at this n the fp32 CPU norm
    the oracle would form from an fp32 gradient is off by 3.5e-5 (measured), which the 1e-5 gate on m and v sees."""
    pr, mr, vr, er = p.clone(), torch.zeros_like(p), torch.zeros_like(p), p.clone()
    for step in range(1, steps + 1):
        gc = O.clip_grad_norm([g.double()], max_norm)[0][0].float() if max_norm > 0 else g
        pr, mr, vr = O.adam_step(pr, gc, mr, vr, step, LR, B1, B2, EPS, wd)
        er = O.ema_update(er, pr, TAU)
        if carry_clipped:
            g = gc
    return pr, mr, vr, er


def _adam_close(got, ref):
    pd, md, vd, ed = got[:4]
    pr, mr, vr, er = ref
    np.testing.assert_allclose(pd.cpu().numpy(), pr.numpy(), rtol=5e-7, atol=2e-7)
    if ed is not None:
        np.testing.assert_allclose(ed.cpu().numpy(), er.numpy(), rtol=5e-7, atol=2e-7)
    assert rel_l2(md, mr) < 1e-5 and rel_l2(vd, vr) < 1e-5


def test_adam_ema_weight_decay_on_a_wrapped_grid(ops, adam_inputs):
    p, _, g = adam_inputs
    got = _adam_gpu(ops, p, g, 0.01, 1.0, True, True)
    assert got[5][0] > 1.0                                   # the clip is active
    _adam_close(got, _adam_ref(p, g, 0.01, 1.0))


def test_adam_ema_inactive_clip_is_no_clip(ops, adam_inputs):
    """norm < max_norm: the coefficient is exactly 1, so the step equals the one without a norm buffer bit for bit."""
    p, g, _ = adam_inputs
    a = _adam_gpu(ops, p, g, 0.0, 100.0, True, True)
    assert a[5][0] < 100.0
    b = _adam_gpu(ops, p, g, 0.0, 0.0, False, True)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    _adam_close(a, _adam_ref(p, g, 0.0, 0.0))


def test_adam_without_ema(ops, adam_inputs):
    p, _, g = adam_inputs
    a = _adam_gpu(ops, p, g, 0.01, 1.0, True, False)
    assert a[3] is None
    _adam_close(a, _adam_ref(p, g, 0.01, 1.0))
    b = _adam_gpu(ops, p, g, 0.01, 1.0, True, True)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


def test_adam_writes_the_clipped_gradient(ops, adam_inputs):
    """write_clipped_grad: g becomes g * coef, coef = max_norm / (norm + 1e-6) formed in fp32 from the norm the device holds
    (2 ulp: rtol 2.4e-7); the second step clips the already clipped gradient again, as the reference is made to do."""
    p, g, _ = adam_inputs
    got = _adam_gpu(ops, p, g, 0.0, 1.0, True, True, write_g=True)
    want = g
    for step in range(2):
        coef = min(np.float32(1.0) / (np.float32(got[5][step]) + np.float32(1e-6)), np.float32(1.0))
        assert step or coef < 0.1                        # the first step clips for real
        want = want * torch.tensor(coef, dtype=torch.float32)
        np.testing.assert_allclose(got[4][step].numpy(), want.numpy(), rtol=2.4e-7, atol=0)
    _adam_close(got, _adam_ref(p, g, 0.0, 1.0, carry_clipped=True))


# ---------------------------------------------------------------------------------------------------
# pointers that are not 16-byte aligned
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("which", ["all", "a", "out"])
def test_axpby_unaligned(ops, with_b, accumulate, which):
    n = 1003
    a, b, prev = gen(n, seed=760), gen(n, seed=761), gen(n, seed=762)
    ad = off1(a) if which in ("all", "a") else a.to(DEV)
    bd = (off1(b) if which == "all" else b.to(DEV)) if with_b else None
    out = off1(prev) if which in ("all", "out") else prev.to(DEV)
    if not accumulate:
        out.fill_(NAN)
    ops.axpby(ad, 0.5, bd, -2.0, out, accumulate=accumulate)
    ref = 0.5 * a.double() + (-2.0 * b.double() if with_b else 0.0) + (prev.double() if accumulate else 0.0)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("L", [256, 512, 1024])
def test_softmax_rows_unaligned(ops, L):
    """At L = 256 / 512 / 1024 an aligned row lives in registers; an unaligned pointer takes the generic kernel."""
    rows = 37
    s, gy = gen(rows, L, seed=66) * 4, gen(rows, L, seed=67)
    y = off1(torch.full((rows, L), NAN))
    ops.softmax_rows(off1(s), y, rows, L)
    ref = F.softmax(s.double(), dim=-1)
    assert rel_l2(y, ref) < 1e-6
    dx = off1(torch.full((rows, L), NAN))
    ops.softmax_rows_bwd(y, off1(gy), dx, rows, L)
    refdx = ref * (gy.double() - (ref * gy.double()).sum(-1, keepdim=True))
    assert rel_l2(dx, refdx) < 1e-5
    # one unaligned operand is enough
    y2 = nan(rows, L)
    ops.softmax_rows(off1(s), y2, rows, L)
    assert rel_l2(y2, ref) < 1e-6
    dx2 = nan(rows, L)
    ops.softmax_rows_bwd(y2, off1(gy), dx2, rows, L)
    assert rel_l2(dx2, refdx) < 1e-5


@pytest.mark.parametrize("co,taps,ci,ns,layout,shift", [(8, 9, 6, 3, 1, 0), (1001, 1, 1, 4, 0, 0), (16, 9, 64, 5, 1, 1),
                                                        (16, 9, 64, 5, 0, 1)],
                         ids=["stem-cin6-oihw", "n1001", "oihw-pointer+1", "flat-pointer+1"])
def test_reduce_slabs_scalar_kernel(ops, co, taps, ci, ns, layout, shift):
    n = co * taps * ci
    slabs = gen(ns, n, seed=770 + co)
    sd = off1(slabs) if shift else slabs.to(DEV)
    out = nan(n)
    ops.reduce_slabs(sd, ns, n, out, layout=layout, cout=co, taps=taps, cin=ci, alpha=0.7)
    ref = 0.7 * slabs.double().sum(0)
    if layout == 1:
        ref = ref.view(co, taps, ci).permute(0, 2, 1).reshape(-1)         # [co][tap][ci] -> OIHW
    assert rel_l2(out, ref) < 1e-6
