"""The 4x4 level of the four-level CIFAR-10 networks on the GPU: the Winograd F(2x2, 3x3) limb kernels on 4x4 maps (seven
images per workgroup: forward / data gradient, every arithmetic; eight images per K tile: weight gradient) against fp64 torch
and the exact limb-product probes, where they read and write (tests/guard.py), the ``c10_ablation`` / ``c10_vpsde`` networks
and the ``clf_c10`` classifier against the reference's forward (tests/golden/net_c10_*.npz) and the CPU oracle's gradients
with the Winograd forms forced on and off, and the command-line drivers with the two presets."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psld_oracle as O
from psld_amd import config as C
from tests import f16_ref as H
from tests import guard as G
from tests import limb_probe as P
from tests import x3_ref as X
from tests.conftest import GOLDEN
from tests.synth import synth_inputs, synth_state_dict
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)
from tests.test_bounds_gpu import guard, pool  # noqa: F401  (fixtures)
from tests.test_kernels_gpu import _nhwc, gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.from_numpy
S = 4
GATE = 3e-6         # the project's gate for the limb kernels against fp64


@pytest.fixture(autouse=True)
def _switches_back_to_default():
    """Whatever a test (or a command-line driver it calls in-process) switched: the process leaves every test with the three
    Winograd switches at their defaults - the tests collected after this file run the default routes."""
    from psld_amd import ops as o
    yield
    o.set_winograd(None)
    o.set_wgrad_winograd(None)
    o.set_winograd_4x4(0)
    assert o.winograd_4x4() == 0


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# forward and data gradient at 4x4
# ---------------------------------------------------------------------------------------------------------------------
FWD = [
    dict(b=1, c1=256, c2=0, co=256),       # one image in a workgroup, 24 of its tiles masked
    dict(b=9, c1=128, c2=0, co=128),       # a full workgroup (seven images) and a partial one
    dict(b=2, c1=256, c2=256, co=256),     # two sources: the up path's unmaterialised concatenation
    dict(b=3, c1=160, c2=0, co=160),       # channel tail
]


def _fwd_data(b, c1, c2, co):
    x = gen(b, c1 + c2, S, S, seed=40)
    w = gen(co, c1 + c2, 3, 3, seed=41, scale=0.05)
    bias, res, temb = gen(co, seed=42), gen(b, co, S, S, seed=43), gen(b, co, seed=44)
    return x, w, bias, res, temb


@pytest.mark.parametrize("cfg", FWD, ids=lambda c: "{b}x{c1}+{c2}->{co}".format(**c))
def test_conv3x3_forward_4x4(ops, cfg):
    """Forward with the full epilogue (bias, time-embedding row bias, residual, scale) against fp64, into a NaN-filled output,
    repeatable bit for bit."""
    b, c1, c2, co = (cfg[n] for n in ("b", "c1", "c2", "co"))
    x, w, bias, res, temb = _fwd_data(b, c1, c2, co)
    ref = (F.conv2d(x.double(), w.double(), bias.double(), padding=1) + temb.double()[:, :, None, None] + res.double()) * 0.7
    x1 = _nhwc(x[:, :c1]).to(DEV)
    x2 = _nhwc(x[:, c1:]).to(DEV) if c2 else None
    epi = ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=S * S, residual=_nhwc(res).to(DEV),
                       ld_residual=co, out_scale=0.7)
    assert ops.conv3x3_wino_supported(c1, c2, b, S, S, co)
    uf = ops.conv3x3_wino_frag(w.to(DEV), False)

    def run():
        y = _nan(b, S, S, co)
        ops.conv3x3_wino(x1, x2, uf, co, y, epi)
        return y
    y = run()
    assert bool(torch.isfinite(y).all())
    err = rel_l2(y.permute(0, 3, 1, 2), ref)
    print(f"wino 4x4 {cfg}: rel-L2 {err:.2e}")
    assert err < GATE
    assert torch.equal(y, run())


def test_conv3x3_forward_4x4_split_chunks(ops):
    """The split-chunk form forced at (b = 8, 512 -> 256) - two pixel tiles x two channel tiles, the 16 chunks over 8
    workgroups each - with the full epilogue and with accumulate, against fp64, repeatable."""
    b, c1, co = 8, 512, 256
    assert ops.conv3x3_wino_ws_bytes(c1, 0, b, S, S, co) > 0, "the split-chunk path is what this case is about"
    x, w, bias, res, temb = _fwd_data(b, c1, 0, co)
    conv = F.conv2d(x.double(), w.double(), padding=1)
    ref = (conv + bias.double()[None, :, None, None] + temb.double()[:, :, None, None] + res.double()) * 0.7
    x1 = _nhwc(x).to(DEV)
    uf = ops.conv3x3_wino_frag(w.to(DEV), False)
    epi = ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=S * S, residual=_nhwc(res).to(DEV),
                       ld_residual=co, out_scale=0.7)
    y1, y2 = _nan(b, S, S, co), _nan(b, S, S, co)
    ops.conv3x3_wino(x1, None, uf, co, y1, epi, allow_split=True)
    ops.conv3x3_wino(x1, None, uf, co, y2, epi, allow_split=True)
    assert rel_l2(y1.permute(0, 3, 1, 2), ref) < GATE and torch.equal(y1, y2)
    # the unsplit launch of the same shape agrees to rounding (another summation order over the chunks)
    y3 = _nan(b, S, S, co)
    ops.conv3x3_wino(x1, None, uf, co, y3, epi)
    assert rel_l2(y3.permute(0, 3, 1, 2), ref) < GATE
    acc = torch.ones(b, S, S, co, device=DEV)
    ops.conv3x3_wino(x1, None, uf, co, acc, ops.epilogue(alpha=0.5, accumulate=True), allow_split=True)
    assert rel_l2(acc.permute(0, 3, 1, 2), conv * 0.5 + 1.0) < GATE


def test_fused_groupnorm_and_partial_sums_stay_refused_at_4x4(ops):
    """The GroupNorm-fused staging needs one image per workgroup region and the partial sums one 64-row run per entry: neither
    holds for a 16-pixel image, and both are refused rather than computed wrongly."""
    assert not ops.conv3x3_wino_gn_supported(256, 0, 8, S, S, 256)
    assert not ops.gn_part_supported(8, S * S, 256)


@pytest.mark.parametrize("b,ci,co", [(1, 256, 256), (9, 128, 256)])
def test_conv3x3_dgrad_4x4(ops, b, ci, co):
    """Data gradient (rotated, role-swapped filter) with the backward tape's alpha / accumulate epilogue."""
    x = gen(b, ci, S, S, seed=60).requires_grad_(True)
    w = gen(co, ci, 3, 3, seed=61, scale=0.05).requires_grad_(True)
    y = F.conv2d(x.double(), w.double(), padding=1)
    gy = gen(*y.shape, seed=62)
    y.backward(gy.double())
    gyd = _nhwc(gy).to(DEV)
    frag = ops.conv3x3_wino_frag(w.detach().to(DEV), True)
    dx = _nan(b, S, S, ci)
    ops.conv3x3_wino(gyd, None, frag, ci, dx, allow_split=True)
    assert rel_l2(dx.permute(0, 3, 1, 2), x.grad) < GATE
    prev = gen(b, S, S, ci, seed=63).to(DEV)
    acc = prev.clone()
    ops.conv3x3_wino(gyd, None, frag, ci, acc, ops.epilogue(alpha=0.5, accumulate=True), allow_split=True)
    assert rel_l2(acc.permute(0, 3, 1, 2), 0.5 * x.grad + prev.permute(0, 3, 1, 2).cpu().double()) < GATE


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient at 4x4
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad_ref(b, ci1, ci2, co, seed):
    x = gen(b, ci1 + ci2, S, S, seed=seed)
    gy = gen(b, co, S, S, seed=seed + 1)
    xr = x.double().requires_grad_(True)
    w = torch.zeros(co, ci1 + ci2, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w, padding=1).backward(gy.double())
    return x, gy, w.grad


@pytest.mark.parametrize("b,ci1,ci2,co", [(8, 256, 0, 256), (16, 256, 256, 256), (24, 384, 0, 512)])
def test_conv3x3_wgrad_4x4(ops, b, ci1, ci2, co):
    """Winograd-domain weight gradient (a K tile = eight images): a single K tile, two sources over two K tiles, three K tiles
    of three c_in tiles; fp64 within 3e-6, repeatable, every K split the shape has, accumulate."""
    x, gy, ref = _wgrad_ref(b, ci1, ci2, co, 80)
    assert ops.conv3x3_wgrad_wino_supported(co, ci1, ci2, b, S, S)
    x1 = _nhwc(x[:, :ci1]).to(DEV)
    x2 = _nhwc(x[:, ci1:]).to(DEV) if ci2 else None
    dyd = _nhwc(gy).to(DEV)
    for ns in (None, 1, b // 8):
        dw = _nan(co, ci1 + ci2, 3, 3)
        ops.conv3x3_wgrad_wino(dyd, co, x1, dw, x2=x2, nsplit=ns)
        err = rel_l2(dw, ref)
        print(f"wgrad 4x4 {b}x{ci1}+{ci2}->{co} nsplit={ns}: {err:.2e}")
        assert err < GATE, ns
        dw2 = _nan(co, ci1 + ci2, 3, 3)
        ops.conv3x3_wgrad_wino(dyd, co, x1, dw2, x2=x2, nsplit=ns)
        assert torch.equal(dw, dw2)
    prev = gen(co, ci1 + ci2, 3, 3, seed=89).to(DEV)
    acc = prev.clone()
    ops.conv3x3_wgrad_wino(dyd, co, x1, acc, x2=x2, accumulate=True, alpha=0.5)
    assert rel_l2(acc, 0.5 * ref + prev.cpu().double()) < GATE


# ---------------------------------------------------------------------------------------------------------------------
# the other arithmetics, and the exact limb products
# ---------------------------------------------------------------------------------------------------------------------
def test_conv3x3_forward_4x4_two_limbs(ops):
    """bf16x3 (two limbs, three products) against tests/x3_ref.py at the gates of test_conv3x3_wino_x3_forward."""
    b, c1, co = 9, 256, 256
    x, w, bias, res, temb = _fwd_data(b, c1, 0, co)
    emu, conv64 = X.two_limb_conv3x3(x, w), F.conv2d(x.double(), w.double(), padding=1)
    x1, uf = _nhwc(x).to(DEV), ops.conv3x3_wino_frag_x3(w.to(DEV))
    y = _nan(b, S, S, co)
    ops.conv3x3_wino_x3(x1, None, uf, co, y)
    e_emu, e_64, emu_64 = rel_l2(y.permute(0, 3, 1, 2), emu), rel_l2(y.permute(0, 3, 1, 2), conv64), rel_l2(emu, conv64)
    print(f"wino x3 4x4: vs two-limb reference {e_emu:.2e}, vs fp64 {e_64:.2e} (reference vs fp64 {emu_64:.2e})")
    assert e_emu <= GATE
    assert 1e-6 < e_64 <= 2 * emu_64
    epi = ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=S * S, residual=_nhwc(res).to(DEV),
                       ld_residual=co, out_scale=0.7)
    ref = (emu + bias.double()[None, :, None, None] + temb.double()[:, :, None, None] + res.double()) * 0.7
    ys = [_nan(b, S, S, co), _nan(b, S, S, co)]
    for yy in ys:
        ops.conv3x3_wino_x3(x1, None, uf, co, yy, epi, allow_split=True)
    assert rel_l2(ys[0].permute(0, 3, 1, 2), ref) <= GATE and torch.equal(*ys)


def test_conv3x3_forward_4x4_fp16(ops):
    """One fp16 product against tests/f16_ref.py at the gates of test_conv3x3_wino_f16_forward, and the operand-shifted form
    (the recording passes' data gradient) at shift 0 and 3."""
    b, c1, co = 9, 256, 256
    x, w, bias, res, temb = _fwd_data(b, c1, 0, co)
    emu, conv64 = H.f16_conv3x3(x, w), F.conv2d(x.double(), w.double(), padding=1)
    x1, uf = _nhwc(x).to(DEV), ops.conv3x3_wino_frag_f16(w.to(DEV))
    y = _nan(b, S, S, co)
    ops.conv3x3_wino_f16(x1, None, uf, co, y)
    e_emu, e_64, emu_64 = rel_l2(y.permute(0, 3, 1, 2), emu), rel_l2(y.permute(0, 3, 1, 2), conv64), rel_l2(emu, conv64)
    print(f"wino f16 4x4: vs fp16 reference {e_emu:.2e}, vs fp64 {e_64:.2e} (reference vs fp64 {emu_64:.2e})")
    assert e_emu <= GATE
    assert 0.5 * emu_64 <= e_64 <= 2 * emu_64
    epi = ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=S * S, residual=_nhwc(res).to(DEV),
                       ld_residual=co, out_scale=0.7)
    ref = (emu + bias.double()[None, :, None, None] + temb.double()[:, :, None, None] + res.double()) * 0.7
    ye = _nan(b, S, S, co)
    ops.conv3x3_wino_f16(x1, None, uf, co, ye, epi, allow_split=True)
    assert rel_l2(ye.permute(0, 3, 1, 2), ref) <= GATE
    y0, y3 = _nan(b, S, S, co), _nan(b, S, S, co)
    ops.conv3x3_wino_f16s(x1, None, uf, co, y0, 0)
    ops.conv3x3_wino_f16s(x1, None, uf, co, y3, 3)
    assert torch.equal(y0, y)                                       # shift 0 is the unshifted kernel bit for bit
    assert rel_l2(y3.permute(0, 3, 1, 2), emu) <= GATE              # in range, a power-of-two shift changes no rounding


def _must_equal(tag, y, launch):
    want = launch.expected(P.PRODUCTS)
    y = y.detach().double().cpu().reshape(want.shape)
    if not torch.equal(y, want):
        pytest.fail(P.explain(tag, y, launch, P.PRODUCTS), pytrace=False)


@pytest.mark.parametrize("dgrad", [False, True], ids=["forward", "dgrad"])
def test_conv3x3_wino_probe_4x4(ops, dgrad):
    """tests/limb_probe.py's exact six-product probe at (b = 9, 128 -> 128): every output element of both workgroups equals the
    model bit for bit - a limb product missing, doubled or taken from a neighbouring tile would show."""
    b, c, co = 9, 128, 128
    for i, la in enumerate(P.wino_launches(b, c, co, S, S, seed=4)):
        w_eff = la.inp["w"]
        wt = (w_eff.flip(2, 3).transpose(0, 1).contiguous() if dgrad else w_eff).to(DEV)
        y = _nan(b, S, S, co)
        ops.conv3x3_wino(_nhwc(la.inp["x"]).to(DEV), None, ops.conv3x3_wino_frag(wt, dgrad), co, y)
        _must_equal(f"wino 4x4 {'data gradient' if dgrad else 'forward'} launch {i}", y, la)


@pytest.mark.parametrize("way", ["dy_pixel", "x_pixel"])
def test_conv3x3_wgrad_wino_probe_4x4(ops, way):
    """The weight gradient's exact probe at (b = 8, 128 -> 256), one K tile: every lit (c_out, c_in, tap) equals the model bit for
    bit, every other one is zero."""
    b, ci, co = 8, 128, 256
    for i, la in enumerate(P.wwino_launches(b, ci, co, S, S, way, seed=4)):
        dw = _nan(co, ci, 3, 3)
        ops.conv3x3_wgrad_wino(_nhwc(la.inp["dy"]).to(DEV), co, _nhwc(la.inp["x"]).to(DEV), dw)
        _must_equal(f"wgrad wino 4x4 {way} launch {i}", dw, la)


# ---------------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------------
def _R(*shape, seed, scale=1.0):
    return gen(*shape, seed=seed, scale=scale).to(DEV)


@pytest.mark.parametrize("b,c,split", [(1, 256, False), (9, 128, False), (9, 128, True), (1, 256, True)])
def test_bounds_forward_4x4(ops, guard, b, c, split):
    t = dict(x1=_R(b, S, S, c, seed=40), bias=_R(c, seed=43), rowbias=_R(b, c, seed=44), res=_R(b, S, S, c, seed=45),
             y=_nan(b, S, S, c), frag=ops.conv3x3_wino_frag(_R(c, c, 3, 3, seed=42, scale=0.05), False))

    def fn(x1, bias, rowbias, res, y, frag):
        epi = ops.epilogue(bias=bias, rowbias=rowbias, rows_per_img=S * S, residual=res, ld_residual=c, out_scale=0.7)
        ops.conv3x3_wino(x1, None, frag, c, y, epi, allow_split=split)
    G.run_guarded(guard, fn, t, ["y"])
    if split:
        assert guard.workspace_calls >= 1 or ops.conv3x3_wino_ws_bytes(c, 0, b, S, S, c) == 0


@pytest.mark.parametrize("b,ci,co,accumulate", [(1, 256, 256, False), (9, 128, 256, True)])
def test_bounds_dgrad_4x4(ops, guard, b, ci, co, accumulate):
    t = dict(gy=_R(b, S, S, co, seed=62), frag=ops.conv3x3_wino_frag(_R(co, ci, 3, 3, seed=61, scale=0.05), True),
             dx=_R(b, S, S, ci, seed=63) if accumulate else _nan(b, S, S, ci))

    def fn(gy, frag, dx):
        ops.conv3x3_wino(gy, None, frag, ci, dx, ops.epilogue(alpha=0.5, accumulate=True) if accumulate else None, allow_split=True)
    G.run_guarded(guard, fn, t, ["dx"])


@pytest.mark.parametrize("c2", [0, 128])
def test_bounds_wgrad_4x4(ops, guard, c2):
    b, c1, co = 8, 256, 256
    t = dict(gy=_R(b, S, S, co, seed=84), x1=_R(b, S, S, c1, seed=83) + 0.25, x2=(_R(b, S, S, c2, seed=85) if c2 else None),
             dw=_nan(co, c1 + c2, 3, 3))

    def fn(gy, x1, x2, dw):
        ops.conv3x3_wgrad_wino(gy, co, x1, dw, x2=x2)
    G.run_guarded(guard, fn, t, ["dw"])
    assert guard.workspace_calls >= 1


# ---------------------------------------------------------------------------------------------------------------------
# the networks
# ---------------------------------------------------------------------------------------------------------------------
def _meta():
    with open(os.path.join(GOLDEN, "c10abl_meta.json")) as fh:
        return json.load(fh)


def _build(name, train=False, dropout=None):
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    meta = _meta()[name]
    cfg = getattr(C, name)()
    if dropout is not None:
        cfg.model.score_fn.dropout = dropout
    net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    net.train(train)
    return net, cfg, sd


@pytest.mark.parametrize("mode", ["wino2", "wino0"])
@pytest.mark.parametrize("name", ["c10_ablation", "c10_vpsde"])
def test_forward_matches_reference(golden, name, mode):
    from psld_amd import ops
    net, cfg, _ = _build(name)
    g = golden(f"net_{name}.npz")
    x, t = T(g["x"]).to(DEV), T(g["t"]).to(DEV)
    try:
        ops.set_winograd(int(mode[-1]))
        ops.set_winograd_4x4(int(mode[-1]))          # (the 4x4 level's own opt-in: 2 every shape, 1 from batch 8, 0 tile engine)
        with torch.no_grad():
            y = net(x, t)
    finally:
        ops.set_winograd(None)
        ops.set_winograd_4x4(0)
    err = rel_l2(y, T(g["y"]))
    print(f"{name} {mode}: rel-L2 vs reference = {err:.3e}")
    assert y.shape == g["y"].shape and err < 2e-5


def test_winograd_reaches_the_4x4_level(monkeypatch):
    """With both forms forced on, one recorded step of c10_ablation at B = 8 launches Winograd kernels on 4x4 maps (one of the
    forward launches with a second source) and sends no 3x3 convolution of 128 or more channels there to the tile engine."""
    from psld_amd import ops
    from psld_amd.registry import get_module
    seen = {"wino": [], "wgrad": [], "tile": []}
    wino, wgrad, conv, cwgrad = ops.conv3x3_wino, ops.conv3x3_wgrad_wino, ops.conv2d_nhwc, ops.conv2d_wgrad_nhwc

    def rec_wino(x1, x2, *a, **k):
        if x1.shape[1] == S:
            seen["wino"].append((x1.shape[-1], x2.shape[-1] if x2 is not None else 0))
        return wino(x1, x2, *a, **k)

    def rec_wgrad(dy, cout, x, dw, x2=None, **k):
        if x.shape[1] == S:
            seen["wgrad"].append((x.shape[-1], x2.shape[-1] if x2 is not None else 0))
        return wgrad(dy, cout, x, dw, x2=x2, **k)

    def rec_conv(x1, x2, w_ohwi, cout, kh, kw, stride, pad, *a, **k):
        if kh == 3 and stride == 1 and x1.shape[1] == S and x1.shape[-1] >= 128:
            seen["tile"].append(("conv", x1.shape[-1], cout))
        return conv(x1, x2, w_ohwi, cout, kh, kw, stride, pad, *a, **k)

    def rec_cwgrad(dy, cout, x, kh, kw, stride, *a, **k):
        if kh == 3 and stride == 1 and x.shape[1] == S and x.shape[-1] >= 128:
            seen["tile"].append(("wgrad", x.shape[-1], cout))
        return cwgrad(dy, cout, x, kh, kw, stride, *a, **k)
    monkeypatch.setattr(ops, "conv3x3_wino", rec_wino)
    monkeypatch.setattr(ops, "conv3x3_wgrad_wino", rec_wgrad)
    monkeypatch.setattr(ops, "conv2d_nhwc", rec_conv)
    monkeypatch.setattr(ops, "conv2d_wgrad_nhwc", rec_cwgrad)
    ops.set_winograd(2)
    ops.set_wgrad_winograd(2)
    ops.set_winograd_4x4(2)
    try:
        net, cfg, _ = _build("c10_ablation", train=True, dropout=0.0)
        sde = get_module("sde", "psld")(cfg)
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        x0, eps, t = synth_inputs(8, 3, 32, seed=5)
        crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV)).backward()
        torch.cuda.synchronize()
    finally:
        ops.set_winograd(None)
        ops.set_wgrad_winograd(None)
        ops.set_winograd_4x4(0)
    print({k: sorted(set(v)) for k, v in seen.items()})
    assert not seen["tile"], seen["tile"]
    # 16 forward launches (nres = 2), and per convolution one data gradient (two for a two-source block)
    assert len(seen["wgrad"]) == 16 and (256, 256) in seen["wino"] and (256, 256) in seen["wgrad"]
    assert len(seen["wino"]) >= 32


def _grads_against_oracle(net, loss, oloss, osd, tag):
    assert abs(loss.item() - oloss.item()) < 2e-5 * abs(oloss.item())
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
    print(f"{tag}: global grad rel-L2 {np.sqrt(num / den):.3e}; worst {worst:.3e} ({worst_k})")
    assert np.sqrt(num / den) < 2e-5
    assert worst < 1e-4, (worst, worst_k)


@pytest.mark.parametrize("mode", [2, 1], ids=["every-shape", "measured-policy"])
def test_c10_ablation_gradients_against_live_oracle(mode):
    """Every parameter gradient at B = 8 (dropout 0) against torch autograd through the oracle on the CPU, at the gates of
    test_full_size_network_gradients_against_live_oracle - the 4x4 level's forward, data and weight gradients in Winograd form:
    ``mode`` 2 with both Winograd switches at 2 (every supported shape at every level), ``mode`` 1 with every switch at its
    policy setting (what ``--winograd-4x4 1`` runs: batch 8 is the first the 4x4 policy takes)."""
    from psld_amd import ops, score_routes as R
    from psld_amd.registry import get_module
    ops.set_winograd(mode)
    ops.set_wgrad_winograd(mode)
    ops.set_winograd_4x4(mode)
    try:
        assert R.conv3_route(True, 256, 256, 8, 4, 4, 256) == R.WINO and R.wgrad_route(True, 256, 256, 256, 8, 4, 4, False) == R.WINO
        assert mode == 2 or R.conv3_route(True, 256, 0, 7, 4, 4, 256) == R.TILE
        net, cfg, sd = _build("c10_ablation", train=True, dropout=0.0)
        sde = get_module("sde", "psld")(cfg)
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        x0, eps, t = synth_inputs(8, 3, 32, seed=321)
        loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
        loss.backward()
    finally:
        ops.set_winograd(None)
        ops.set_wgrad_winograd(None)
        ops.set_winograd_4x4(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
    oloss = O.psld_score_loss(O.PSLDOracle.from_config(cfg), x0, t, lambda z, tt: O.ncsnpp_forward(osd, cfg, z, tt), eps)
    oloss.backward()
    _grads_against_oracle(net, loss, oloss, osd, f"c10_ablation (mode {mode})")


def test_c10_vpsde_eval_forward_at_batch_8_under_the_measured_policy():
    """``set_winograd_4x4(1)`` with the other switches at their defaults, B = 8 (the first batch the policy takes): the eval
    forward against the oracle's at the gate of the full-network forwards, and against the default route's output."""
    from psld_amd import ops
    net, cfg, sd = _build("c10_vpsde")
    g = torch.Generator().manual_seed(19)
    x = torch.randn(8, 3, 32, 32, generator=g)
    t = torch.rand(8, generator=g) * 0.98 + 0.01
    with torch.no_grad():
        y0 = net(x.to(DEV), t.to(DEV))
        ops.set_winograd_4x4(1)
        try:
            y1 = net(x.to(DEV), t.to(DEV))
        finally:
            ops.set_winograd_4x4(0)
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        ref = O.ncsnpp_forward(sd, cfg, x, t)
    e0, e1 = rel_l2(y0, ref), rel_l2(y1, ref)
    print(f"c10_vpsde B=8: default {e0:.3e}, 4x4 policy on {e1:.3e}")
    assert e0 < 2e-5 and e1 < 2e-5
    assert not torch.equal(y0, y1), "the opt-in changed no launch"


def test_clf_c10_forward_and_input_gradient_against_oracle():
    """The guidance classifier (ch_mult [1,2,3,4]: 384 -> 512 and 512 -> 512 on 4x4 maps) at B = 8, Winograd forced on: logits
    and d(sum of selected logits)/dx against the oracle at the gates of test_classifier_logits_and_input_gradient."""
    import psld_amd
    from psld_amd import ops
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    ccfg = C.clf_c10()
    ccfg.model.clf_fn.dropout = 0.0
    clf = get_module("clf_fn", "ncsnpp_clf")(ccfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in clf.state_dict().items()], 23)
    clf.load_state_dict(sd, strict=True)
    clf = clf.to(DEV).eval()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(8, 6, 32, 32, generator=g)
    t = torch.rand(8, generator=g) * 0.98 + 0.01
    sel = torch.randn(8, 10, generator=g)
    ops.set_winograd(2)
    ops.set_wgrad_winograd(2)
    ops.set_winograd_4x4(2)
    try:
        xd = x.to(DEV).requires_grad_()
        logits = clf(xd, t.to(DEV))
        (gx,) = torch.autograd.grad(logits, xd, grad_outputs=sel.to(DEV))
    finally:
        ops.set_winograd(None)
        ops.set_wgrad_winograd(None)
        ops.set_winograd_4x4(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    xo = x.clone().requires_grad_()
    ologits = O.ncsnpp_clf_forward(sd, ccfg, xo, t)
    (ogx,) = torch.autograd.grad(ologits, xo, grad_outputs=sel)
    e1, e2 = rel_l2(logits, ologits), rel_l2(gx, ogx)
    print(f"clf_c10: logits {e1:.3e}, input gradient {e2:.3e}")
    assert e1 < 2e-5 and e2 < 1e-4


def test_c10_vpsde_vjp_input_is_the_autograd_dx():
    """NCSNpp.vjp_input (the likelihood's input-gradient-only backward) through the 4x4 level at B = 8: bitwise the full
    backward's dx."""
    from psld_amd import ops
    net, cfg, _ = _build("c10_vpsde")
    g = torch.Generator().manual_seed(11)
    x = torch.randn(8, 3, 32, 32, generator=g).to(DEV)
    t = (torch.rand(8, generator=g) * 0.9 + 0.05).to(DEV)
    w = torch.randn(8, 3, 32, 32, generator=g).to(DEV)
    ops.set_winograd(2)
    ops.set_wgrad_winograd(2)
    ops.set_winograd_4x4(2)
    try:
        y, dx = net.vjp_input(x, t, w)
        xr = x.clone().requires_grad_()
        y_full = net(xr, t)
        y_full.backward(w)
    finally:
        ops.set_winograd(None)
        ops.set_wgrad_winograd(None)
        ops.set_winograd_4x4(0)
    assert torch.equal(y, y_full.detach())
    assert torch.equal(dx, xr.grad), f"rel-L2 {rel_l2(dx, xr.grad):.3e}"
    assert float(dx.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_bpd_takes_the_presets(capsys):
    """``bpd --config c10_vpsde`` / ``c10_ablation`` in-process: two synthetic images, the freshly initialised network, a loose
    solve - one JSON line each with a finite figure."""
    import math

    from psld_amd import cli
    for name in ("c10_vpsde", "c10_ablation"):
        cli.main(["bpd", "--config", name, "--synthetic-size", "2", "--max-images", "2", "--rtol", "1e-2", "--atol", "1e-2",
                  "evaluation.batch_size=2"])
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
        out = json.loads(line)
        assert out["n_images"] == 2 and math.isfinite(out["bpd"]) and out["mean_nfe"] > 0, (name, out)


def test_cli_train_c10_ablation_and_sample_c10_vpsde(tmp_path):
    """``train --config c10_ablation --winograd-4x4 1`` for 2 steps on 16 synthetic images writes a checkpoint; ``sample --config
    c10_vpsde --winograd-4x4 2`` from a two-step c10_vpsde checkpoint writes 2 images after 3 steps.  The flag holds for its own
    call only: a call without it runs (and leaves the process) at 0."""
    from psld_amd import cli, ops
    res, out = str(tmp_path / "run"), str(tmp_path / "s")
    try:
        cli.main(["train", "--config", "c10_ablation", "--winograd-4x4", "1", "--max-steps", "2", "--synthetic-size", "16",
                  "--log-every", "1", "dataset.diffusion.training.batch_size=8", "dataset.diffusion.training.epochs=1",
                  f"dataset.diffusion.training.results_dir='{res}'", "training.chkpt_prefix=t"])
        assert ops.winograd_4x4() == 1
        sd = torch.load(os.path.join(res, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=False)
        assert sd["global_step"] == 2
        # a VP-SDE checkpoint to sample from: two steps of the same driver, no flag
        res2 = str(tmp_path / "run2")
        cli.main(["train", "--config", "c10_vpsde", "--max-steps", "2", "--synthetic-size", "16", "--log-every", "1",
                  "dataset.diffusion.training.batch_size=8", "dataset.diffusion.training.epochs=1",
                  f"dataset.diffusion.training.results_dir='{res2}'", "training.chkpt_prefix=t"])
        assert ops.winograd_4x4() == 0
        ck = os.path.join(res2, "checkpoints", "last.ckpt")
        cli.main(["sample", "--config", "c10_vpsde", "--winograd-4x4", "2", f"evaluation.chkpt_path={ck}", "evaluation.n_samples=2",
                  "evaluation.batch_size=2", "evaluation.n_discrete_steps=3", f"evaluation.save_path={out}",
                  "evaluation.save_mode=np", "evaluation.sample_prefix=gpu"])
        assert ops.winograd_4x4() == 2
    finally:
        ops.set_winograd_4x4(0)
    img_dir = os.path.join(out, "1000", "images")           # the preset carries the sampling script's path_prefix
    files = sorted(os.listdir(img_dir))
    assert files
    for f in files:
        a = np.load(os.path.join(img_dir, f))
        assert a.dtype == np.uint8 and a.shape == (2, 32, 32, 3)
