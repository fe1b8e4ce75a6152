"""Record math 'bf16x3' on the GPU: the two-limb Winograd-domain weight gradient, the two-limb data-gradient fragments and
the pointwise data gradient on two limbs against the CPU reference of the arithmetic (tests/x3_train_ref.py, fp64
accumulation: the kernels differ from it in fp32 summation order only, the project's 3e-6 kernel gate); networks trained
under the setting against the live oracle (the 1e-4 parity contract), what the executor dispatches, weight caches, the
captured training step and guard-band runs of the new entry points.  Every test restores the process's settings."""
import contextlib
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psld_oracle as O
from psld_amd import config as C
from tests import guard as G
from tests import x3_ref as X
from tests import x3_train_ref as XT
from tests.synth import synth_inputs, synth_state_dict
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)
from tests.test_bounds_gpu import guard, pool  # noqa: F401  (fixtures)
from tests.test_kernels_gpu import _nhwc, gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@contextlib.contextmanager
def record_math(record, mode="bf16x6", winograd=2, wgrad=2):
    """Record math ``record`` under math mode ``mode`` with Winograd forward / data gradient / weight gradient forced."""
    from psld_amd import ops as o
    old, old_r = o.math_mode(), o.record_math()
    try:
        o.set_math_mode(mode)
        o.set_record_math(record)
        o.set_winograd(winograd)
        o.set_wgrad_winograd(wgrad)
        yield
    finally:
        o.set_winograd(None)
        o.set_wgrad_winograd(None)
        o.set_record_math(old_r)
        o.set_math_mode(old)


def _checks(tag, y2, y3, emu, ref64):
    """The gates every two-limb launch meets: y2 against the two-limb reference and true fp64, and apart from three limbs."""
    e_emu, e_64, emu_64 = rel_l2(y2, emu), rel_l2(y2, ref64), rel_l2(emu, ref64)
    print(f"{tag}: vs two-limb reference {e_emu:.2e}, vs fp64 {e_64:.2e} (reference vs fp64 {emu_64:.2e}), "
          f"three-limb launch vs fp64 {rel_l2(y3, ref64):.2e}")
    assert e_emu < 3e-6
    assert 1e-6 < e_64 < 1e-4
    assert not torch.equal(y2, y3)


# ---------------------------------------------------------------------------------------------------------------------
# Winograd-domain weight gradient, two limbs
# ---------------------------------------------------------------------------------------------------------------------
WGRAD = [
    dict(b=8, c1=128, c2=0, co=256, s=8, nsplit=2),
    dict(b=4, c1=256, c2=0, co=256, s=16, nsplit=1),
    dict(b=2, c1=128, c2=0, co=256, s=32, nsplit=None),
    dict(b=1, c1=128, c2=0, co=128, s=64, nsplit=None),       # the CO = 128 instance
    dict(b=1, c1=128, c2=0, co=128, s=128, nsplit=None),      # a K tile is half a tile row
    dict(b=3, c1=256, c2=128, co=256, s=32, nsplit=3),        # two sources, odd batch
    dict(b=10, c1=256, c2=0, co=256, s=32, nsplit=7),         # the last split is shorter
    dict(b=2, c1=160, c2=0, co=160, s=16, nsplit=None),       # tails
    dict(b=2, c1=160, c2=0, co=256, s=16, nsplit=None),
    dict(b=2, c1=128, c2=160, co=320, s=16, nsplit=None),
]


@pytest.mark.parametrize("cfg", WGRAD, ids=lambda c: "{b}x{c1}+{c2}->{co}@{s}".format(**c))
def test_conv3x3_wgrad_wino_x3(ops, cfg):
    b, c1, c2, co, s, ns = (cfg[n] for n in ("b", "c1", "c2", "co", "s", "nsplit"))
    ci = c1 + c2
    assert ops.conv3x3_wgrad_wino_supported(co, c1, c2, b, s, s)
    xt = gen(b, ci, s, s, seed=83) + 0.25                   # a mean: the transforms cancel it, the limbs must carry it
    gyt = gen(b, co, s, s, seed=84)
    w = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt.double(), w, padding=1).backward(gyt.double())
    emu = XT.two_limb_wgrad3x3(xt, gyt)
    x1 = _nhwc(xt[:, :c1]).to(DEV)
    x2 = _nhwc(xt[:, c1:]).to(DEV) if c2 else None
    gy = _nhwc(gyt).to(DEV)
    dw = torch.full((co, ci, 3, 3), float("nan"), device=DEV)
    ops.conv3x3_wgrad_wino_x3(gy, co, x1, dw, x2=x2, nsplit=ns)
    dw3 = torch.full_like(dw, float("nan"))
    ops.conv3x3_wgrad_wino(gy, co, x1, dw3, x2=x2, nsplit=ns)
    _checks("wgrad x3 {b}x{c1}+{c2}->{co}@{s}".format(**cfg), dw, dw3, emu, w.grad)
    again = torch.full_like(dw, float("nan"))
    ops.conv3x3_wgrad_wino_x3(gy, co, x1, again, x2=x2, nsplit=ns)
    assert torch.equal(again, dw)
    acc = torch.ones_like(dw)
    ops.conv3x3_wgrad_wino_x3(gy, co, x1, acc, x2=x2, nsplit=ns, accumulate=True)
    assert torch.equal(acc, dw + 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# data gradient of the 3x3 convolutions: two-limb fragments of the rotated, transposed weights
# ---------------------------------------------------------------------------------------------------------------------
def _planes(buf, limbs, payload):
    return buf[:payload].view(torch.int32).reshape(-1, limbs, 256)


@pytest.mark.parametrize("co,ci", [(256, 128), (320, 160), (256, 384)])
def test_wino_dgrad_packer_planes(ops, co, ci):
    """The planes are the hi and mid planes of the three-limb data-gradient fragments, bit for bit; the batched packer takes a
    data-gradient row (its table carries the strides and the flip) and writes what the single launch writes."""
    w = gen(co, ci, 3, 3, seed=11, scale=0.05).to(DEV)
    f3, f2 = ops.conv3x3_wino_frag(w, True), ops.conv3x3_wino_dgrad_frag_x3(w)
    assert f2.numel() == ops.conv3x3_wino_frag_bytes_x3(ci, co) == co * ci * 64 + 16384
    assert torch.equal(_planes(f2, 2, co * ci * 64), _planes(f3, 3, co * ci * 96)[:, :2])
    outs = [torch.zeros_like(f2), torch.zeros_like(ops.conv3x3_wino_frag_x3(w))]
    rows = [ops.conv3x3_wino_frag_entry(w, True, outs[0]) + [0], ops.conv3x3_wino_frag_entry(w, False, outs[1]) + [co * ci // 8]]
    ops.pack_wino_batch_x3(torch.tensor(rows, dtype=torch.int64, device=DEV), 2, 2 * (co * ci // 8))
    assert torch.equal(outs[0][:co * ci * 64], f2[:co * ci * 64])
    assert torch.equal(outs[1][:co * ci * 64], ops.conv3x3_wino_frag_x3(w)[:co * ci * 64])


@pytest.mark.parametrize("co,ci,b,s", [(256, 128, 4, 16), (320, 160, 2, 16)])
def test_conv3x3_dgrad_on_two_limb_fragments(ops, co, ci, b, s):
    """dx = conv3x3_wino_x3(dy, data-gradient fragments): ``co`` channels of dy to ``ci`` channels of dx."""
    wt = gen(co, ci, 3, 3, seed=41, scale=0.05)
    dyt = gen(b, co, s, s, seed=40)
    x64 = torch.zeros(b, ci, s, s, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, wt.double(), padding=1).backward(dyt.double())
    emu = XT.two_limb_dgrad3x3(dyt, wt)
    dy, w = _nhwc(dyt).to(DEV), wt.to(DEV)
    f2, f3 = ops.conv3x3_wino_dgrad_frag_x3(w), ops.conv3x3_wino_frag(w, True)
    nan = torch.full((b, s, s, ci), float("nan"), device=DEV)

    def run(e, init, split=True):
        y = init.clone()
        ops.conv3x3_wino_x3(dy, None, f2, ci, y, e, allow_split=split)
        return y
    y = run(None, nan)
    y3 = nan.clone()
    ops.conv3x3_wino(dy, None, f3, ci, y3, None, allow_split=True)
    _checks(f"dgrad x3 {b}x{co}->{ci}@{s}", y.permute(0, 3, 1, 2), y3.permute(0, 3, 1, 2), emu, x64.grad)
    assert torch.equal(y, run(None, nan))
    acc = run(ops.epilogue(accumulate=True), torch.ones_like(nan))
    assert torch.equal(acc, y + 1.0)


def test_conv3x3_dgrad_per_source_slices_on_two_limbs(ops):
    """One source's share of the data gradient of a convolution that reads a 128 + 256 concatenation: a contiguous slice of the
    two-limb fragments (ordered by 16-channel block of dx), as _resblock_cat_bwd cuts the three-limb ones."""
    b, s, co, c1, c2 = 2, 16, 256, 128, 256
    ci = c1 + c2
    wt = gen(co, ci, 3, 3, seed=43, scale=0.05)
    dyt = gen(b, co, s, s, seed=44)
    emu = XT.two_limb_dgrad3x3(dyt, wt)
    dy, w = _nhwc(dyt).to(DEV), wt.to(DEV)
    f2 = ops.conv3x3_wino_dgrad_frag_x3(w)
    cut = (f2.numel() - 16384) * c1 // ci
    whole = torch.full((b, s, s, ci), float("nan"), device=DEV)
    ops.conv3x3_wino_x3(dy, None, f2, ci, whole, None)
    assert rel_l2(whole.permute(0, 3, 1, 2), emu) < 3e-6
    for lo, hi, fr in ((0, c1, f2[:cut]), (c1, ci, f2[cut:])):
        part = torch.full((b, s, s, hi - lo), float("nan"), device=DEV)
        ops.conv3x3_wino_x3(dy, None, fr, hi - lo, part, None)
        err = rel_l2(part.permute(0, 3, 1, 2), emu[:, lo:hi])
        print(f"dgrad x3 source [{lo}:{hi}] of {ci}: {err:.2e}")
        assert err < 3e-6
        assert torch.equal(part, whole[..., lo:hi])          # a channel's result does not depend on who shares its launch


# ---------------------------------------------------------------------------------------------------------------------
# pointwise data gradient on two limbs
# ---------------------------------------------------------------------------------------------------------------------
def test_pointwise_dgrad_on_two_limbs(ops):
    """dx[m][512] = dy[m][256] W for a 1x1 convolution weight stored [256 out][512 in] (the [k][n] orientation: stride_n = 1,
    stride_k = 512) at m = 16 x 32 x 32, and the share of its second 256 input channels from the fragments' second half."""
    m, k, n = 16 * 32 * 32, 256, 512
    wt = gen(k, n, seed=51, scale=0.05)                     # [out = k of the data gradient][in = n]
    dyt = gen(m, k, seed=50)
    emu, ref64 = X.two_limb_matmul(dyt, wt.t()), dyt.double() @ wt.double()
    assert ops.gemm_split_x3_wanted(k, 0, m, n) and ops.gemm_split_x3_wanted(k, 0, m, 256)
    dy, w = dyt.to(DEV), wt.to(DEV)
    f2, f3 = ops.gemm_frag_x3(w, n, k, 1, n), ops.gemm_frag(w, n, k, 1, n)
    assert torch.equal(_planes(f2, 2, n * k * 4), _planes(f3, 3, n * k * 6)[:, :2])
    nan = torch.full((m, n), float("nan"), device=DEV)

    def run(e, init, frag=f2, width=n):
        y = init.clone()
        ops.gemm_split_x3(dy, None, m, frag, width, y, e)
        return y
    y = run(None, nan)
    y3 = nan.clone()
    ops.gemm_split(dy, None, m, f3, n, y3, None)
    _checks("pointwise dgrad x3 256->512", y, y3, emu, ref64)
    assert torch.equal(y, run(None, nan))
    assert torch.equal(run(ops.epilogue(accumulate=True), torch.ones_like(nan)), y + 1.0)
    # columns 256 .. 512: the second half of the fragments
    half = f2[f2.numel() // 2:]
    nan2 = torch.full((m, 256), float("nan"), device=DEV)
    part = run(None, nan2, half, 256)
    y3h = nan2.clone()
    ops.gemm_split(dy, None, m, f3[f3.numel() // 2:], 256, y3h, None)
    _checks("pointwise dgrad x3 256->512, columns 256:512", part, y3h, emu[:, 256:], ref64[:, 256:])
    assert torch.equal(part, run(None, nan2, half, 256))
    assert torch.equal(run(ops.epilogue(accumulate=True), torch.ones_like(nan2), half, 256), part + 1.0)


def _attention_harness(c, seed=78):
    """tests/test_blocks_gpu.py's Harness around one attention block of ``c`` channels (built under the current settings)."""
    from psld_amd import score_fn as S
    from tests.test_blocks_gpu import Harness
    mod = S.AttnBlockpp(c)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in mod.state_dict().items()], seed)
    return Harness(mod, sd), sd


def test_qkv_data_gradient_set_on_two_limbs(ops):
    """The shared q | k | v data-gradient set of an attention block at c = 256 as the executor builds it (NCSNpp._qkv_frags_x3:
    three parameters placed along K = 3c by the batched packer's chunk placement): its planes are the hi and mid planes of the
    three-limb set, it equals the two-limb fragments of the concatenated matrix, the launch pw_dgrad issues on it
    (m = 16384 rows: the smallest the policy gives to the two-limb kernel at this width) meets the kernel gates, and after the
    weights change the batched refresh of the 'limb_x3' family fills it anew."""
    c, m = 256, 16384
    assert ops.gemm_split_x3_wanted(3 * c, 0, m, c) and not ops.gemm_split_x3_wanted(3 * c, 0, m - 128, c)
    p2, p3 = 3 * c * c * 4, 3 * c * c * 6
    with record_math("bf16x3"):
        h, _ = _attention_harness(c)
        net, mod = h.net, h.mod
        nins = (mod.NIN_0, mod.NIN_1, mod.NIN_2)

        def sets():
            wcat = torch.cat([n_.W.detach() for n_ in nins], dim=1).contiguous()     # B[n = c in][k = 3c out]
            pd3, pd2 = net._qkv_frags(mod)[1], net._qkv_frags_x3(mod, True)
            assert torch.equal(_planes(pd2, 2, p2), _planes(pd3, 3, p3)[:, :2])
            assert torch.equal(pd2[:p2], ops.gemm_frag_x3(wcat, c, 3 * c, 3 * c, 1)[:p2])
            return wcat, pd2, pd3
        wcat, pd2, pd3 = sets()
        dt = gen(m, 3 * c, seed=60)
        d = dt.to(DEV)
        emu, ref64 = X.two_limb_matmul(dt, wcat.cpu()), dt.double() @ wcat.cpu().double().t()
        nan = torch.full((m, c), float("nan"), device=DEV)

        def run(e, init):
            y = init.clone()
            ops.gemm_split_x3(d, None, m, pd2, c, y, e)
            return y
        y = run(None, nan)
        y3 = nan.clone()
        ops.gemm_split(d, None, m, pd3, c, y3, None)
        _checks("q|k|v data gradient x3, 768->256", y, y3, emu, ref64)
        assert torch.equal(y, run(None, nan))
        assert torch.equal(run(ops.epilogue(accumulate=True), torch.ones_like(nan)), y + 1.0)
        # the weights move (as under the fused optimizer: written in place, then weights_changed): the entries are refreshed
        # together by the family's one launch, into the same buffers
        before, ptr = pd2.clone(), pd2.data_ptr()
        tags = {tag for _, tag in net._wcache.entries}
        assert {"qkv_set_d_x3", "qkv_d_x3"} <= tags, sorted(tags)
        with torch.no_grad():
            for i, n_ in enumerate(nins):
                n_.W.add_(gen(c, c, seed=61 + i, scale=0.02).to(DEV))
        net.weights_changed()
        wcat_b, pd2_b, _ = sets()
        assert pd2_b.data_ptr() == ptr and not torch.equal(pd2_b, before) and not torch.equal(wcat_b, wcat)
        y_b = run(None, nan)
        assert rel_l2(y_b, X.two_limb_matmul(dt, wcat_b.cpu())) < 3e-6


def test_attention_block_backward_at_the_width_the_two_limb_set_takes(monkeypatch):
    """One attention block at c = 256 on 16x16 maps, B = 64 (m = 16384: pw_dgrad takes the two-limb q | k | v data-gradient set
    and the two-limb NIN_3 fragments), forward and every gradient against the oracle: below 1e-4 each (the parity contract) and
    apart from the 'bf16x6' run.  The launch log holds the K = 3c data-gradient launch on two limbs and no three-limb pointwise
    launch the policy gives to two limbs."""
    from psld_amd import ops as o
    c, hw, b = 256, 16, 64
    g = torch.Generator().manual_seed(6)
    x = torch.randn(b, c, hw, hw, generator=g)
    gy = torch.randn(b, c, hw, hw, generator=g)
    got = {}
    for record in ("bf16x6", "bf16x3"):
        with record_math(record):
            h, sd = _attention_harness(c)
            assert ("x3" in h.ex.arith) == (record == "bf16x3")
            log = []
            for name in ("gemm_split", "gemm_split_x3"):
                def rec(*a, _fn=getattr(o, name), _name=name, **k):
                    k2 = a[0].shape[-1] + (a[1].shape[-1] if a[1] is not None else 0)
                    log.append((_name, k2, a[4], o.gemm_split_x3_wanted(k2, 0, a[2], a[4])))
                    return _fn(*a, **k)
                monkeypatch.setattr(o, name, rec)
            xn = h.S._Node(x.permute(0, 2, 3, 1).contiguous().to(DEV))
            with h.ops.stream_scope():
                out = h.ex.attn(xn, h.mod)
            h.backward(out, gy.permute(0, 2, 3, 1).contiguous().to(DEV))
            monkeypatch.undo()
            got[record] = ([("y", out.v.permute(0, 3, 1, 2).clone()), ("dx", xn.g.permute(0, 3, 1, 2).clone())]
                           + [(k, h.grad(k).clone()) for k in sd], log)
    osd = {f"m.{k}": v.double().requires_grad_(True) for k, v in sd.items()}
    xo = x.double().requires_grad_(True)
    yo = O.attn_block(xo, osd, "m")
    yo.backward(gy.double())
    ref = dict([("y", yo), ("dx", xo.grad)] + [(k, osd[f"m.{k}"].grad) for k in sd])
    (t3, log3), (t6, log6) = got["bf16x3"], got["bf16x6"]
    print("launches under record math bf16x3:", sorted(set(log3)))
    assert ("gemm_split_x3", 3 * c, c, True) in log3                        # the q | k | v data gradient
    assert ("gemm_split_x3", c, 3 * c, True) in log3 and ("gemm_split_x3", c, c, True) in log3
    assert not [r for r in log3 if r[0] == "gemm_split" and r[3]]
    assert log6 and not [r for r in log6 if r[0] == "gemm_split_x3"]
    bq = dict(t3)["NIN_0.b"].abs().max().item()
    for (k, a3), (_, a6) in zip(t3, t6):
        if k == "NIN_1.b":          # analytically zero (softmax is shift-invariant): against the query bias's gradient
            assert a3.abs().max().item() < 1e-4 * bq
            continue
        e3, e6 = rel_l2(a3, ref[k]), rel_l2(a6, ref[k])
        print(f"attention 256 @16 B=64 under record math bf16x3: {k} {e3:.2e} (bf16x6 {e6:.2e})")
        assert e3 < 1e-4, k
        if k in ("y", "dx"):
            assert not torch.equal(a3, a6), k


def test_pyramid_data_gradient_on_two_limbs():
    """The input pyramid's 3x3 stride-2 convolution 256 -> 256 from 16x16 maps at B = 32 (m = 2048 rows, 9 x 256 columns of
    patches: 144 tiles, the two-limb kernel's) as the executor runs it - im2col GEMM, data gradient on the 's2dgrad_x3'
    fragments of the packed weight, col2im - against the oracle's Downsample: below 1e-4 each, dx apart from the 'bf16x6' run."""
    from psld_amd import ops as o
    from psld_amd import score_fn as S
    from tests.test_blocks_gpu import Harness
    c, hw, b = 256, 16, 32
    assert o.gemm_split_x3_wanted(c, 0, b * (hw // 2) ** 2, 9 * c)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(b, c, hw, hw, generator=g)
    gy = torch.randn(b, c, hw // 2, hw // 2, generator=g)
    got = {}
    for record in ("bf16x6", "bf16x3"):
        with record_math(record):
            mod = S.Downsample(c, c, True)
            sd = synth_state_dict([(k, tuple(v.shape)) for k, v in mod.state_dict().items()], 79)
            h = Harness(mod, sd)
            s_ = h.ex.s
            hz = h.S._Node(torch.zeros((b, hw // 2, hw // 2, c), device=DEV))
            pyr = h.S._Node(x.permute(0, 2, 3, 1).contiguous().to(DEV))
            with h.ops.stream_scope():
                out = h.ex.pyramid(pyr, hz, h.mod, False)
            h.backward(out, gy.permute(0, 2, 3, 1).contiguous().to(DEV) / s_)
            tags = {tag for _, tag in h.net._wcache.entries}
            assert ("s2dgrad_x3" in tags) == (record == "bf16x3"), sorted(tags)
            got[record] = [("y", out.v.permute(0, 3, 1, 2) / s_), ("dx", pyr.g.permute(0, 3, 1, 2).clone())] + \
                [(k, h.grad(k).clone()) for k in sd]
    osd = {f"m.{k}": v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    yo = O.pyramid_downsample(xo, osd, "m")
    yo.backward(gy)
    ref = dict([("y", yo), ("dx", xo.grad)] + [(k, osd[f"m.{k}"].grad) for k in sd])
    for (k, a3), (_, a6) in zip(got["bf16x3"], got["bf16x6"]):
        e3, e6 = rel_l2(a3, ref[k]), rel_l2(a6, ref[k])
        print(f"pyramid 256->256 from 16x16, B=32 under record math bf16x3: {k} {e3:.2e} (bf16x6 {e6:.2e})")
        assert e3 < 1e-4, k
    assert not torch.equal(dict(got["bf16x3"])["dx"], dict(got["bf16x6"])["dx"])
    assert 1e-6 < rel_l2(dict(got["bf16x3"])["dx"], ref["dx"])          # two limbs: about 4e-6 (the pointwise kernel's figure)


# ---------------------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------------------
LIMB3 = ("conv3x3_wino", "gemm_split", "conv3x3_wgrad_wino")
LIMB2 = ("conv3x3_wino_x3", "gemm_split_x3", "conv3x3_wgrad_wino_x3")


def _record(monkeypatch, log, phase):
    """Recording wrappers around the limb entry points of ``ops``: (name, phase, a two-limb form would take the shape)."""
    from psld_amd import ops as o
    for name in LIMB3 + LIMB2:
        def rec(*a, _fn=getattr(o, name), _name=name, **k):
            takes = True
            if _name == "gemm_split":
                a1, a2, m, n = a[0], a[1], a[2], a[4]
                takes = o.gemm_split_x3_wanted(a1.shape[-1], a2.shape[-1] if a2 is not None else 0, m, n)
            log.append((_name, phase[0], takes))
            return _fn(*a, **k)
        monkeypatch.setattr(o, name, rec)


def _c10_gradients(log=None, monkeypatch=None):
    """Loss and flat gradient of one C10-SOTA pass at B = 2, seed 321 (tests/test_model_gpu.py: _full_size_gradients)."""
    from psld_amd.registry import get_module
    from tests.test_model_gpu import _build
    net, cfg, sd = _build("c10_sota", train=True)
    cfg.model.score_fn.dropout = 0.0
    net.sf.dropout = 0.0
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    x0, eps, t = synth_inputs(2, 3, cfg.data.image_size, seed=321)
    phase = ["forward"]
    if log is not None:
        _record(monkeypatch, log, phase)
    loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
    phase[0] = "backward"
    loss.backward()
    if log is not None:
        monkeypatch.undo()
    return net, cfg, sd, (x0, eps, t), loss


def test_c10_gradients_against_live_oracle_under_record_math(monkeypatch):
    """Every parameter gradient of C10-SOTA (B = 2) under record math 'bf16x3' against torch autograd through the oracle.
    Global rel-L2 below 1e-4 (the parity contract; CPU estimate of the arithmetic 7.5e-6); the worst tensor by
    test_model_gpu's damped measure is printed, not gated (CPU estimate 6.8e-5; measured on an MI355X: global 8.16e-6, worst
    tensor 7.1e-5, all_modules.32.Conv_1.weight).  The gradients differ from the 'bf16x6'
    run, forward / data-gradient / weight-gradient launches are the two-limb ones and no three-limb launch runs where a
    two-limb one exists."""
    import os
    with record_math("bf16x6"):
        net6, _, _, _, loss6 = _c10_gradients()
        g6 = net6.flat_grad().clone()
        del net6
    log = []
    with record_math("bf16x3"):
        net, cfg, sd, (x0, eps, t), loss = _c10_gradients(log, monkeypatch)
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    try:
        osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
        oloss = O.psld_score_loss(O.PSLDOracle.from_config(cfg), x0, t, lambda z, tt: O.ncsnpp_forward(osd, cfg, z, tt), eps)
        oloss.backward()
    finally:
        torch.set_num_threads(threads)
    total = torch.stack([v.grad.double().norm() for v in osd.values() if v.grad is not None]).norm().item()
    worst, worst_k, num, den = 0.0, None, 0.0, 0.0
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        a, bb = p.grad.double().cpu(), osd[k].grad.double()
        e = ((a - bb).norm() / (bb.norm() + 1e-4 * total)).item()
        num += float((a - bb).pow(2).sum())
        den += float(bb.pow(2).sum())
        if e > worst:
            worst, worst_k = e, k
    d6 = rel_l2(net.flat_grad(), g6)
    print(f"c10_sota under record math bf16x3: loss {loss.item():.6f} (oracle {oloss.item():.6f}, bf16x6 {loss6.item():.6f}); "
          f"global grad rel-L2 {np.sqrt(num / den):.3e}; worst tensor {worst:.3e} ({worst_k}); vs the bf16x6 gradients {d6:.3e}")
    assert abs(loss.item() - oloss.item()) < 1e-4 * abs(oloss.item())
    assert np.sqrt(num / den) < 1e-4
    assert not torch.equal(net.flat_grad(), g6) and d6 < 1e-4
    names = {(n, p) for n, p, _ in log}
    print("launches:", {k: sum(1 for n, p, _ in log if (n, p) == k) for k in sorted(names)})
    assert ("conv3x3_wino_x3", "forward") in names and ("conv3x3_wino_x3", "backward") in names
    assert ("conv3x3_wgrad_wino_x3", "backward") in names
    assert not [r for r in log if r[0] in ("conv3x3_wino", "conv3x3_wgrad_wino")]
    assert not [r for r in log if r[0] == "gemm_split" and r[2]]


def test_pointwise_launches_at_b16_under_record_math(monkeypatch):
    """C10-SOTA at B = 16: the pointwise forward and data-gradient GEMMs the two-limb kernel takes (128 tiles and more: the 1x1
    shortcuts of the 32x32 level, with their per-source column slices) run on it in a recording pass, in both limb math modes; with record math 'bf16x6' none of the two-limb entry points is called.  The gradients of the
    two-limb passes lie within 1e-4 (the parity contract; 7.7e-6 at B = 2) of the three-limb pass's - before and after an
    optimizer step, which the two-limb data-gradient entries of the 'limb_x3' / 'wino_x3' families follow through their batched
    refresh: a fresh network loaded with the stepped weights gives the same gradients bit for bit."""
    from psld_amd.optim import FusedAdam
    from psld_amd.registry import get_module
    from tests.test_model_gpu import _build
    net, cfg, _ = _build("c10_sota", train=True)
    cfg.model.score_fn.dropout = 0.0
    net.sf.dropout = 0.0
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    x0, eps, t = (v.to(DEV) for v in synth_inputs(16, 3, 32, seed=5))

    def grads(n_, record, mode, log=None):
        phase = ["forward"]
        for p in n_.parameters():
            p.grad = None
        with record_math(record, mode):
            if log is not None:
                _record(monkeypatch, log, phase)
            loss = crit(x0, t, n_, eps=eps)
            phase[0] = "backward"
            loss.backward()
            if log is not None:
                monkeypatch.undo()
        return n_.flat_grad().clone()
    flat = {}
    for record, mode in (("bf16x3", "bf16x6"), ("bf16x3", "bf16x3"), ("bf16x6", "bf16x3")):
        log = []
        flat[record, mode] = grads(net, record, mode, log)
        names = {(n, p) for n, p, _ in log}
        print(f"record math {record}, math mode {mode}:", {k: sum(1 for n, p, _ in log if (n, p) == k) for k in sorted(names)})
        if record == "bf16x6":
            assert log and not [r for r in log if r[0] in LIMB2]
            continue
        for want in (("gemm_split_x3", "forward"), ("gemm_split_x3", "backward"), ("conv3x3_wino_x3", "forward"),
                     ("conv3x3_wino_x3", "backward"), ("conv3x3_wgrad_wino_x3", "backward")):
            assert want in names, want
        assert not [r for r in log if r[0] in ("conv3x3_wino", "conv3x3_wgrad_wino")]
        assert not [r for r in log if r[0] == "gemm_split" and r[2]]
    g6 = flat["bf16x6", "bf16x3"]
    for mode in ("bf16x6", "bf16x3"):
        d = rel_l2(flat["bf16x3", mode], g6)
        print(f"B = 16 gradients, record math bf16x3 under math mode {mode} vs record math bf16x6: {d:.3e}")
        assert not torch.equal(flat["bf16x3", mode], g6) and d < 1e-4
    tags = {tag for _, tag in net._wcache.entries}
    assert {"wfrag_d_x3", "dgrad_x3", "fwd_x3"} <= tags, sorted(tags)
    # one optimizer step on the last gradient (the three-limb pass's), then the same comparison on the moved weights
    FusedAdam(net, lr=1e-3, grad_clip=1.0).step()
    g3b, g6b = grads(net, "bf16x3", "bf16x6"), grads(net, "bf16x6", "bf16x6")
    d = rel_l2(g3b, g6b)
    print(f"B = 16 gradients after an optimizer step: {d:.3e}; the step moved them by {rel_l2(g6b, g6):.3e}")
    assert not torch.equal(g6b, g6) and not torch.equal(g3b, g6b) and d < 1e-4
    fresh = get_module("score_fn", "ncsnpp")(cfg)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    fresh = fresh.to(DEV).train()
    fresh.sf.dropout = 0.0
    assert torch.equal(grads(fresh, "bf16x3", "bf16x6"), g3b)


def test_tail_width_resblock_against_the_oracle_under_record_math():
    """One residual block 160 -> 320 on 16x16 maps (channel tails in every kernel): output and all gradients against the
    oracle, global rel-L2 below 1e-4 each and over everything."""
    from psld_amd import score_fn as S
    from tests.test_blocks_gpu import Harness, _nchw
    cin, cout, hw, b = 160, 320, 16, 2
    with record_math("bf16x3"):
        mod = S.ResnetBlockBigGANpp(cin, cout, temb_dim=128, dropout=0.0)
        sd = synth_state_dict([(k, tuple(v.shape)) for k, v in mod.state_dict().items()], 77)
        g = torch.Generator().manual_seed(5)
        x, temb = torch.randn(b, cin, hw, hw, generator=g), torch.randn(b, 128, generator=g)
        h = Harness(mod, sd)
        assert "x3" in h.ex.arith
        h.set_temb(temb)
        xin = h.S._Node(x.permute(0, 2, 3, 1).contiguous().to(DEV))
        with h.ops.stream_scope():
            out = h.ex.resblock(xin, h.mod)
        osd = {f"m.{k}": v.clone().requires_grad_(True) for k, v in sd.items()}
        xo, to = x.clone().requires_grad_(True), temb.clone().requires_grad_(True)
        yo = O.resblock_biggan(xo, to, osd, "m")
        gy = torch.randn(*yo.shape, generator=g)
        yo.backward(gy)
        h.backward(out, gy.permute(0, 2, 3, 1).contiguous().to(DEV))
        pairs = [("y", _nchw(out.v), yo), ("dx", _nchw(xin.g), xo.grad), ("dtemb", h.temb_grad(), to.grad)]
        pairs += [(k, h.grad(k), osd[f"m.{k}"].grad) for k in sd]
    num = den = 0.0
    for k, a, r in pairs:
        e = rel_l2(a, r)
        print(f"resblock 160->320 @16 under record math bf16x3: {k} {e:.2e}")
        assert e < 1e-4, k
        if k != "y":
            num += float((a.detach().double().cpu() - r.double()).pow(2).sum())
            den += float(r.double().pow(2).sum())
    print(f"all gradients, global rel-L2 {np.sqrt(num / den):.3e}")
    assert 1e-7 < np.sqrt(num / den) < 1e-4


def _tiny128(attn=True):
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    cfg = C.tiny(nf=128, ch_mult=(1, 1), attn_resolutions=(16,) if attn else (8,))
    sde = get_module("sde", "psld")(cfg)
    return cfg, sde, get_module


def test_training_overfits_fixed_batch_under_record_math():
    """150 steps on one fixed batch (tests/test_model_gpu.py: test_training_overfits_fixed_batch) on the 128-channel tiny
    network with attention on its 16x16 maps: the last loss below half the first; the 'bf16x6' run's is printed beside it."""
    from psld_amd.optim import FusedAdam
    cfg, sde, get_module = _tiny128()
    x0, eps, t = (v.to(DEV) for v in synth_inputs(8, 3, 16, seed=5))
    last = {}
    for record in ("bf16x6", "bf16x3"):
        with record_math(record):
            torch.manual_seed(0)
            net = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
            crit = get_module("losses", "psld_score_loss")(cfg, sde)
            opt = FusedAdam(net, lr=1e-3, grad_clip=1.0)
            losses = []
            for _ in range(150):
                loss = crit(x0, t, net, eps=eps)
                loss.backward()
                opt.step()
                losses.append(loss.detach())
            losses = torch.stack(losses).cpu().numpy()
        assert np.isfinite(losses).all()
        last[record] = (float(losses[0]), float(losses[-1]))
    print(f"overfit, 150 steps: record math bf16x3 {last['bf16x3'][0]:.4f} -> {last['bf16x3'][1]:.3e}; "
          f"bf16x6 {last['bf16x6'][0]:.4f} -> {last['bf16x6'][1]:.3e}")
    assert last["bf16x3"][1] < 0.5 * last["bf16x3"][0], last


def test_weight_caches_follow_the_optimizer_under_record_math():
    """After three optimizer steps with warm two-limb caches (forward, data-gradient and pointwise fragments refreshed by the
    batched packers) a fresh network loaded with the weights agrees bitwise in the next step's gradients."""
    from psld_amd.optim import FusedAdam
    cfg, sde, get_module = _tiny128()
    with record_math("bf16x3"):
        torch.manual_seed(1)
        net = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        opt = FusedAdam(net, lr=1e-3, grad_clip=1.0)
        x0, eps, t = (v.to(DEV) for v in synth_inputs(4, 3, 16, seed=9))
        for _ in range(3):
            crit(x0, t, net, eps=eps).backward()
            opt.step()
        tags = {tag for _, tag in net._wcache.entries}
        assert {"wfrag_x3", "wfrag_d_x3"} <= tags, sorted(tags)
        fresh = get_module("score_fn", "ncsnpp")(cfg)
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
        fresh = fresh.to(DEV).train()
        for n_ in (net, fresh):
            for p_ in n_.parameters():
                p_.grad = None
        torch.manual_seed(5); crit(x0, t, net, eps=eps).backward()
        torch.manual_seed(5); crit(x0, t, fresh, eps=eps).backward()
        assert torch.equal(net.flat_grad(), fresh.flat_grad())
        g3 = net.flat_grad().clone()
    with record_math("bf16x6"):         # the three-limb entries of the same network are their own, and fresh as well
        for p_ in fresh.parameters():
            p_.grad = None
        torch.manual_seed(5); crit(x0, t, fresh, eps=eps).backward()
        assert not torch.equal(fresh.flat_grad(), g3) and rel_l2(fresh.flat_grad(), g3) < 1e-4


def test_graph_captured_training_step_under_record_math():
    """The captured training step under record math 'bf16x3' is bitwise the eager step, and switching the record math between
    steps captures anew instead of replaying the other mode's launches."""
    from psld_amd.optim import EMAWeightUpdate
    cfg, sde, get_module = _tiny128()
    cfg.model.score_fn.dropout = 0.0
    cfg.training.optimizer.warmup = 4
    torch.manual_seed(3)
    net_a = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
    net_b = copy.deepcopy(net_a)
    data = [torch.rand(4, 3, 16, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(i)) * 2 - 1 for i in range(10)]
    # steps 0-4 under 'bf16x3' (two eager warm-up steps, the capture, two replays), steps 5-9 under 'bf16x6' (the same again)
    plan = ["bf16x3"] * 5 + ["bf16x6"] * 5
    runs = []
    for net, graphs in ((net_a, False), (net_b, True)):
        ema = copy.deepcopy(net)
        for p in ema.parameters():
            p.requires_grad = False
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        wr = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema, criterion=crit)
        if graphs:
            wr.enable_graphs(True, warmup_steps=2)
        cb = EMAWeightUpdate(cfg.training.ema_decay)
        torch.manual_seed(11)
        losses = []
        for i, record in enumerate(plan):
            with record_math(record):
                losses.append(wr.training_step(data[i], i).item())
                cb.on_train_batch_end(None, wr)
        runs.append((losses, net.flatten_parameters().clone(), ema.flatten_parameters().clone()))
        if graphs:
            keys = list(wr._graph_steps)
            assert len(keys) == 2 and {k[3] for k in keys} == {("x3", "x6"), ("x6",)}, keys       # ops.pass_arith(True) of each
            assert all("graph" in e for e in wr._graph_steps.values())
    (la, pa, ea), (lb, pb, eb) = runs
    print("eager  losses", la)
    print("graph  losses", lb)
    assert la == lb and torch.equal(pa, pb) and torch.equal(ea, eb)


# ---------------------------------------------------------------------------------------------------------------------
# guard bands (tests/guard.py): the new entry points on buffers of exactly the documented size
# ---------------------------------------------------------------------------------------------------------------------
def _R(*shape, seed, scale=1.0):
    return gen(*shape, seed=seed, scale=scale).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _guard_wgrad(b, c1, c2, co, s, nsplit, accumulate):
    def build(ops):
        t = dict(gy=_R(b, s, s, co, seed=84), x1=_R(b, s, s, c1, seed=83) + 0.25, x2=(_R(b, s, s, c2, seed=85) if c2 else None),
                 dw=(_R(co, c1 + c2, 3, 3, seed=86) if accumulate else _nan(co, c1 + c2, 3, 3)))

        def fn(gy, x1, x2, dw):             # slabs: ops.workspace of exactly psld_conv3x3_wgrad_wino_ws_bytes
            ops.conv3x3_wgrad_wino_x3(gy, co, x1, dw, x2=x2, nsplit=nsplit, accumulate=accumulate, alpha=0.5 if accumulate else 1.0)
        return fn, t, ["dw"], 1
    return build


def _guard_dgrad_pack(co, ci):
    def build(ops):
        t = dict(w=_R(co, ci, 3, 3, seed=3, scale=0.1),
                 out=torch.zeros(ops.conv3x3_wino_frag_bytes_x3(ci, co), dtype=torch.uint8, device=DEV))
        return (lambda w, out: ops.conv3x3_wino_dgrad_frag_x3(w, out)), t, ["out"], 0
    return build


def _guard_dgrad_conv(co, c_lo, c_hi, ci, b, s):
    """The data gradient's launch on the fragment slice of input channels [c_lo, c_hi) of ``ci``."""
    def build(ops):
        f2 = ops.conv3x3_wino_dgrad_frag_x3(_R(co, ci, 3, 3, seed=3, scale=0.1))
        assert c_hi == ci               # the last source's slice ends with the fragments' read-ahead pad
        fr = f2[(f2.numel() - 16384) * c_lo // ci:].clone()
        t = dict(dy=_R(b, s, s, co, seed=40), fr=fr, dx=_nan(b, s, s, c_hi - c_lo))
        return (lambda dy, fr, dx: ops.conv3x3_wino_x3(dy, None, fr, c_hi - c_lo, dx, None, allow_split=True)), t, ["dx"], 0
    return build


def _guard_pw_dgrad(m, k, n, lo, hi):
    def build(ops):
        f2 = ops.gemm_frag_x3(_R(k, n, seed=51, scale=0.05), n, k, 1, n)
        fr = f2[f2.numel() * lo // n:f2.numel() * hi // n].clone()
        t = dict(dy=_R(m, k, seed=50), fr=fr, dx=_R(m, hi - lo, seed=52))
        return (lambda dy, fr, dx: ops.gemm_split_x3(dy, None, m, fr, hi - lo, dx, ops.epilogue(alpha=0.5, accumulate=True))), t, ["dx"], 0
    return build


GUARDED = {
    "wgrad_x3-2x128->256@32": _guard_wgrad(2, 128, 0, 256, 32, None, False),
    "wgrad_x3-8x128->256@8-ns2": _guard_wgrad(8, 128, 0, 256, 8, 2, False),
    "wgrad_x3-x2-3x256+128->256@32-ns3": _guard_wgrad(3, 256, 128, 256, 32, 3, False),
    "wgrad_x3-acc-1x128->128@64": _guard_wgrad(1, 128, 0, 128, 64, None, True),
    "wgrad_x3-tail-2x160->160@16": _guard_wgrad(2, 160, 0, 160, 16, None, False),
    "wgrad_x3-tail-x2-acc-2x128+160->320@16": _guard_wgrad(2, 128, 160, 320, 16, None, True),
    "pack-wino_dgrad_x3-256x128": _guard_dgrad_pack(256, 128),
    "pack-wino_dgrad_x3-320x160": _guard_dgrad_pack(320, 160),
    "dgrad_x3-4x256->128@16": _guard_dgrad_conv(256, 0, 128, 128, 4, 16),
    "dgrad_x3-2x320->160@16": _guard_dgrad_conv(320, 0, 160, 160, 2, 16),
    "dgrad_x3-2x256->[128:384]@16": _guard_dgrad_conv(256, 128, 384, 384, 2, 16),
    "pw_dgrad_x3-256->512": _guard_pw_dgrad(16 * 32 * 32, 256, 512, 0, 512),
    "pw_dgrad_x3-256->512[256:512]": _guard_pw_dgrad(16 * 32 * 32, 256, 512, 256, 512),
}


@pytest.mark.parametrize("name", list(GUARDED))
def test_bounds_of_the_two_limb_training_launches(ops, guard, name):
    fn, tensors, outputs, min_ws = GUARDED[name](ops)
    torch.cuda.synchronize()
    G.run_guarded(guard, fn, tensors, outputs)
    assert guard.workspace_calls >= min_ws, f"{guard.workspace_calls} guarded workspace calls, expected {min_ws}"
