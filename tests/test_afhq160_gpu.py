"""The AFHQv2-128 inpainting network (nf = 160) on the GPU: the Winograd limb kernels with channel tails (widths that are
multiples of 32 from 128 up, not of 128) against fp64 torch and against themselves on zero-padded channels, the full
network against the reference's forward (net_afhq160.npz) and the CPU oracle's gradients, where the executor sends its 3x3
convolutions, and ``inpaint --config afhqv2_128_inpaint``."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psld_oracle as O
from psld_amd import config as C
from tests.synth import synth_inputs, synth_state_dict
from tests.test_kernels_gpu import _nhwc, gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.from_numpy


@pytest.fixture(scope="module", autouse=True)
def _leave_the_stream_pool_where_it_was():
    """Every network this module builds takes streams from torch's per-device pool, which hands them out round-robin, and
    the runtime spreads those streams over a few hardware queues.  Later tests in the same process that need a stream of their
    own on a queue apart from the compute stream's (test_fullsize_gpu.py's co-residency test) see the pool where the suite
    without this module left it: after the module, streams are taken until the pool is back at its starting position."""
    first = torch.cuda.Stream(device=DEV).cuda_stream
    yield

    def take_until_first():
        for n in range(1, 1025):
            if torch.cuda.Stream(device=DEV).cuda_stream == first:
                return n
        raise AssertionError("stream pool did not wrap around")
    take_until_first()                      # the pool is one past `first`, as after the fixture's own first call
    size = take_until_first()               # once round: the pool's size
    for _ in range(size - 1):               # one short of a second round: where it was before that first call
        torch.cuda.Stream(device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# kernels: channel tails of 32, 64 and 96 (160, 320, 480) at the network's map sizes
# ---------------------------------------------------------------------------------------------------------------------
FWD = [
    dict(b=1, c1=160, c2=0, co=160, s=128),
    dict(b=2, c1=320, c2=160, co=160, s=64),       # two sources, 320 + 160 in
    dict(b=1, c1=160, c2=0, co=320, s=64),
    dict(b=4, c1=320, c2=0, co=480, s=16),
    dict(b=8, c1=480, c2=480, co=480, s=8),
    dict(b=2, c1=480, c2=0, co=320, s=8),
]


def _fwd_ref(b, c1, c2, co, s, seed):
    x = gen(b, c1 + c2, s, s, seed=seed)
    w = gen(co, c1 + c2, 3, 3, seed=seed + 1, scale=0.05)
    bias, res, temb = gen(co, seed=seed + 2), gen(b, co, s, s, seed=seed + 3), gen(b, co, seed=seed + 4)
    return x, w, bias, res, temb


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("cfg", FWD, ids=lambda c: "{b}x{c1}+{c2}->{co}@{s}".format(**c))
def test_conv3x3_wino_forward_channel_tail(ops, cfg, split):
    """Forward with the full epilogue (bias, time-embedding row bias, residual, scale), then with alpha + accumulate, against
    fp64 within 3e-6; every launch repeats bit for bit.  ``split``: the executor's call (allow_split: the split-chunk form
    where the grid is small)."""
    b, c1, c2, co, s = (cfg[n] for n in ("b", "c1", "c2", "co", "s"))
    x, w, bias, res, temb = _fwd_ref(b, c1, c2, co, s, 40)
    assert ops.conv3x3_wino_supported(c1, c2, b, s, s, co)
    ref = (F.conv2d(x.double(), w.double(), bias.double(), padding=1) + temb.double()[:, :, None, None] + res.double()) * 0.7
    x1 = _nhwc(x[:, :c1]).to(DEV)
    x2 = _nhwc(x[:, c1:]).to(DEV) if c2 else None
    uf = ops.conv3x3_wino_frag(w.to(DEV), False)
    epi = ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=s * s, residual=_nhwc(res).to(DEV),
                       ld_residual=co, out_scale=0.7)

    def run(e, init):
        y = init.clone()
        ops.conv3x3_wino(x1, x2, uf, co, y, e, allow_split=split)
        return y
    nan = torch.full((b, s, s, co), float("nan"), device=DEV)
    y = run(epi, nan)
    err = rel_l2(y.permute(0, 3, 1, 2), ref)
    print(f"forward {cfg} split={split}: rel-L2 {err:.2e}")
    assert err < 3e-6
    assert torch.equal(y, run(epi, nan))
    prev = gen(b, s, s, co, seed=49).to(DEV)
    acc = run(ops.epilogue(alpha=0.5, accumulate=True), prev)
    err = rel_l2(acc.permute(0, 3, 1, 2), F.conv2d(x.double(), w.double(), padding=1) * 0.5 + prev.permute(0, 3, 1, 2).cpu().double())
    print(f"forward accumulate {cfg} split={split}: rel-L2 {err:.2e}")
    assert err < 3e-6
    assert torch.equal(acc, run(ops.epilogue(alpha=0.5, accumulate=True), prev))


@pytest.mark.parametrize("b,ci,co,s", [(1, 160, 320, 128), (1, 320, 160, 64), (2, 480, 480, 16), (4, 160, 160, 8)])
def test_conv3x3_wino_dgrad_channel_tail(ops, b, ci, co, s):
    """Data gradient (rotated, role-swapped fragments: the launch's width is the forward's cin) with the backward tape's
    alpha / accumulate epilogue against fp64 autograd within 3e-6, repeatable, split as the executor calls it."""
    x = gen(b, ci, s, s, seed=60).requires_grad_(True)
    w = gen(co, ci, 3, 3, seed=61, scale=0.05).requires_grad_(True)
    y = F.conv2d(x.double(), w.double(), padding=1)
    gy = gen(*y.shape, seed=62)
    y.backward(gy.double())
    gyd = _nhwc(gy).to(DEV)
    assert ops.conv3x3_wino_supported(co, 0, b, s, s, ci)
    frag = ops.conv3x3_wino_frag(w.detach().to(DEV), True)
    dx = torch.full((b, s, s, ci), float("nan"), device=DEV)
    ops.conv3x3_wino(gyd, None, frag, ci, dx, allow_split=True)
    err = rel_l2(dx.permute(0, 3, 1, 2), x.grad)
    print(f"dgrad {b} {ci}<-{co} @{s}: rel-L2 {err:.2e}")
    assert err < 3e-6
    dx2 = torch.full_like(dx, float("nan"))
    ops.conv3x3_wino(gyd, None, frag, ci, dx2, allow_split=True)
    assert torch.equal(dx, dx2)
    prev = gen(b, s, s, ci, seed=63).to(DEV)
    acc = prev.clone()
    ops.conv3x3_wino(gyd, None, frag, ci, acc, ops.epilogue(alpha=0.5, accumulate=True), allow_split=True)
    assert rel_l2(acc.permute(0, 3, 1, 2), 0.5 * x.grad + prev.permute(0, 3, 1, 2).cpu().double()) < 3e-6


@pytest.mark.parametrize("b,c1,co,s", [(1, 320, 320, 16), (1, 640, 320, 8)])
def test_conv3x3_wino_split_chunks_channel_tail_at_b1(ops, b, c1, co, s):
    """The split-chunk form at B = 1 (a grid of a few workgroups: channel chunks over workgroups, one reduction pass with the
    epilogue) against fp64 within 3e-6, repeatable."""
    assert ops.conv3x3_wino_ws_bytes(c1, 0, b, s, s, co) > 0
    x, w, bias, res, _ = _fwd_ref(b, c1, 0, co, s, 70)
    ref = (F.conv2d(x.double(), w.double(), bias.double(), padding=1) + res.double()) * 0.7
    x1 = _nhwc(x).to(DEV)
    uf = ops.conv3x3_wino_frag(w.to(DEV), False)
    epi = ops.epilogue(bias=bias.to(DEV), residual=_nhwc(res).to(DEV), ld_residual=co, out_scale=0.7)
    y1 = torch.full((b, s, s, co), float("nan"), device=DEV)
    ops.conv3x3_wino(x1, None, uf, co, y1, epi, allow_split=True)
    err = rel_l2(y1.permute(0, 3, 1, 2), ref)
    print(f"split chunks {c1}->{co} @{s}: rel-L2 {err:.2e}")
    assert err < 3e-6
    y2 = torch.full_like(y1, float("nan"))
    ops.conv3x3_wino(x1, None, uf, co, y2, epi, allow_split=True)
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("b,c1,co,s", [(1, 160, 160, 128), (2, 320, 480, 16), (1, 640, 160, 8), (4, 480, 320, 8)])
def test_conv3x3_wino_channel_independence(ops, b, c1, co, s):
    """A launch of ``co`` output channels equals, bit for bit, the first ``co`` channels of the same launch with the weights
    (and the epilogue's per-channel operands) zero-padded to the next multiple of 128 - forward and data gradient, split as
    the executor calls it."""
    pad = -(-co // 128) * 128
    x, w, bias, res, temb = _fwd_ref(b, c1, 0, co, s, 80)
    wp = torch.zeros(pad, c1, 3, 3)
    wp[:co] = w
    x1 = _nhwc(x).to(DEV)
    resd = _nhwc(res).to(DEV)
    resp = torch.zeros(b, s, s, pad, device=DEV)
    resp[..., :co] = resd
    biasp, tembp = torch.zeros(pad), torch.zeros(b, pad)
    biasp[:co], tembp[:, :co] = bias, temb
    y = torch.full((b, s, s, co), float("nan"), device=DEV)
    ops.conv3x3_wino(x1, None, ops.conv3x3_wino_frag(w.to(DEV), False), co, y,
                     ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=s * s, residual=resd, ld_residual=co,
                                  out_scale=0.7), allow_split=True)
    yp = torch.full((b, s, s, pad), float("nan"), device=DEV)
    ops.conv3x3_wino(x1, None, ops.conv3x3_wino_frag(wp.to(DEV), False), pad, yp,
                     ops.epilogue(bias=biasp.to(DEV), rowbias=tembp.to(DEV), rows_per_img=s * s, residual=resp, ld_residual=pad,
                                  out_scale=0.7), allow_split=True)
    assert torch.equal(y, yp[..., :co].contiguous())
    # data gradient: the launch's width is the forward's cin (here co: weights [c1][co] as a [out = c1][in = co] conv)
    gy = _nhwc(gen(b, c1, s, s, seed=88)).to(DEV)
    wt = w.transpose(0, 1).contiguous()                  # [c1][co][3][3]: dgrad output width co
    wtp = torch.zeros(c1, pad, 3, 3)
    wtp[:, :co] = wt
    dx = torch.full((b, s, s, co), float("nan"), device=DEV)
    ops.conv3x3_wino(gy, None, ops.conv3x3_wino_frag(wt.to(DEV), True), co, dx, allow_split=True)
    dxp = torch.full((b, s, s, pad), float("nan"), device=DEV)
    ops.conv3x3_wino(gy, None, ops.conv3x3_wino_frag(wtp.to(DEV), True), pad, dxp, allow_split=True)
    assert torch.equal(dx, dxp[..., :co].contiguous())


def _wgrad_ref(b, ci1, ci2, co, s, seed):
    x = gen(b, ci1 + ci2, s, s, seed=seed)
    gy = gen(b, co, s, s, seed=seed + 1)
    xr = x.double().requires_grad_(True)
    w = torch.zeros(co, ci1 + ci2, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w, padding=1).backward(gy.double())
    return x, gy, w.grad


WGRAD = [
    dict(b=1, ci1=160, ci2=0, co=160, s=128),
    dict(b=2, ci1=480, ci2=0, co=160, s=64),
    dict(b=1, ci1=128, ci2=160, co=160, s=64),     # two sources: the second one's last c_in tile cut short
    dict(b=4, ci1=320, ci2=0, co=480, s=16),
    dict(b=16, ci1=480, ci2=0, co=320, s=8),
    dict(b=2, ci1=160, ci2=0, co=256, s=32),       # c_in tail under a 256-channel c_out tile
]


@pytest.mark.parametrize("cfg", WGRAD, ids=lambda c: "{b}x{ci1}+{ci2}->{co}@{s}".format(**c))
def test_conv3x3_wgrad_wino_channel_tail(ops, cfg):
    """Winograd-domain weight gradient with c_out / c_in tails: fp64 within 3e-6 for nsplit in {default, 3}, accumulate,
    repeatable bit for bit."""
    b, ci1, ci2, co, s = (cfg[n] for n in ("b", "ci1", "ci2", "co", "s"))
    x, gy, ref = _wgrad_ref(b, ci1, ci2, co, s, 90)
    assert ops.conv3x3_wgrad_wino_supported(co, ci1, ci2, b, s, s)
    x1 = _nhwc(x[:, :ci1]).to(DEV)
    x2 = _nhwc(x[:, ci1:]).to(DEV) if ci2 else None
    dyd = _nhwc(gy).to(DEV)
    for ns in (None, 3):
        dw = torch.full((co, ci1 + ci2, 3, 3), float("nan"), device=DEV)
        ops.conv3x3_wgrad_wino(dyd, co, x1, dw, x2=x2, nsplit=ns)
        err = rel_l2(dw, ref)
        print(f"wgrad {cfg} nsplit={ns}: rel-L2 {err:.2e}")
        assert err < 3e-6, ns
        dw2 = torch.full_like(dw, float("nan"))
        ops.conv3x3_wgrad_wino(dyd, co, x1, dw2, x2=x2, nsplit=ns)
        assert torch.equal(dw, dw2)
    prev = gen(co, ci1 + ci2, 3, 3, seed=99).to(DEV)
    acc = prev.clone()
    ops.conv3x3_wgrad_wino(dyd, co, x1, acc, x2=x2, accumulate=True, alpha=0.5)
    assert rel_l2(acc, 0.5 * ref + prev.cpu().double()) < 3e-6


@pytest.mark.parametrize("b,ci,co,s", [(1, 160, 160, 128), (4, 480, 320, 16), (16, 160, 480, 8)])
def test_conv3x3_wgrad_wino_channel_independence(ops, b, ci, co, s):
    """The weight gradient's c_out rows and c_in columns do not depend on the launch's width: equal bit for bit to the
    leading block of the same launch on operands zero-padded to 256 channels (same K splits)."""
    x = _nhwc(gen(b, ci, s, s, seed=100)).to(DEV)
    dy = _nhwc(gen(b, co, s, s, seed=101)).to(DEV)
    ns, _ = ops.conv3x3_wgrad_wino_plan(co, ci, b, s, s)
    cp, op = -(-ci // 256) * 256, -(-co // 256) * 256
    xp = torch.zeros(b, s, s, cp, device=DEV)
    xp[..., :ci] = x
    dyp = torch.zeros(b, s, s, op, device=DEV)
    dyp[..., :co] = dy
    dw = torch.full((co, ci, 3, 3), float("nan"), device=DEV)
    ops.conv3x3_wgrad_wino(dy, co, x, dw, nsplit=ns)
    dwp = torch.full((op, cp, 3, 3), float("nan"), device=DEV)
    ops.conv3x3_wgrad_wino(dyp, op, xp, dwp, nsplit=ns)
    assert torch.equal(dw, dwp[:co, :ci].contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# the AFHQv2-128 inpainting network (nf = 160)
# ---------------------------------------------------------------------------------------------------------------------
S = 128


def _meta():
    from tests.conftest import GOLDEN
    with open(os.path.join(GOLDEN, "afhq160_meta.json")) as fh:
        return json.load(fh)


def _build(train=False, dropout=None):
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    meta = _meta()
    cfg = C.afhqv2_128_inpaint()
    if dropout is not None:
        cfg.model.score_fn.dropout = dropout
    net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    net.train(train)
    return net, cfg, sd


@pytest.mark.parametrize("mode", ["wino1", "wino2", "wino0", "f32"])
def test_afhq160_forward_matches_reference(golden, mode):
    """Eval forward of the 128.4 M-parameter network against the reference's (net_afhq160.npz) within 2e-5."""
    from psld_amd import ops
    net, cfg, _ = _build()
    g = golden("net_afhq160.npz")
    x, t = T(g["x"]).to(DEV), T(g["t"]).to(DEV)
    old = ops.math_mode()
    try:
        if mode == "f32":
            ops.set_math_mode("f32")
        else:
            ops.set_winograd(int(mode[-1]))
        with torch.no_grad():
            y = net(x, t)
    finally:
        ops.set_winograd(None)
        ops.set_math_mode(old)
    err = rel_l2(y, T(g["y"]))
    print(f"afhq160 {mode}: rel-L2 vs reference = {err:.3e}")
    assert y.shape == g["y"].shape and err < 2e-5


@pytest.mark.parametrize("winograd,wgrad", [(1, 1), (0, 0)])
def test_afhq160_gradients_against_live_oracle(winograd, wgrad):
    """Every parameter gradient vs torch autograd through the oracle on the CPU (B = 1, dropout 0): the gates of
    test_afhq128_gradients_against_live_oracle."""
    from psld_amd import ops
    from psld_amd.registry import get_module
    ops.set_winograd(winograd)
    ops.set_wgrad_winograd(wgrad)
    try:
        net, cfg, sd = _build(train=True, dropout=0.0)
        sde = get_module("sde", "psld")(cfg)
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        x0, eps, t = synth_inputs(1, 3, S, seed=321)
        loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
        loss.backward()
    finally:
        ops.set_winograd(None)
        ops.set_wgrad_winograd(None)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
    oloss = O.psld_score_loss(O.PSLDOracle.from_config(cfg), x0, t, lambda z, tt: O.ncsnpp_forward(osd, cfg, z, tt), eps)
    oloss.backward()
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
    print(f"afhq160 ({winograd},{wgrad}): global grad rel-L2 {np.sqrt(num / den):.3e}; worst {worst:.3e} ({worst_k})")
    assert np.sqrt(num / den) < 2e-5
    assert worst < 1e-4, (worst, worst_k)


def test_afhq160_dispatch_keeps_limb_widths_off_the_tile_engine(monkeypatch):
    """One training step and one eval forward at B = 4 through the recording wrappers of
    test_afhq128_dispatch_keeps_limb_shapes_off_the_tile_engine: no 3x3 stride-1 convolution whose cin and cout are both
    multiples of 32 from 128 up reaches the fp32 tile engine - forward, data gradient or weight gradient - at any map size."""
    from psld_amd import ops
    from psld_amd.registry import get_module
    tile, tile_wgrad = [], []
    conv, wgrad = ops.conv2d_nhwc, ops.conv2d_wgrad_nhwc

    def rec_conv(x1, x2, w_ohwi, cout, kh, kw, stride, pad, *a, **k):
        tile.append((x1.shape[-1] + (x2.shape[-1] if x2 is not None else 0), cout, kh, stride, x1.shape[2]))
        return conv(x1, x2, w_ohwi, cout, kh, kw, stride, pad, *a, **k)

    def rec_wgrad(dy, cout, x, kh, kw, stride, *a, **k):
        tile_wgrad.append((x.shape[-1], cout, kh, stride, x.shape[2]))
        return wgrad(dy, cout, x, kh, kw, stride, *a, **k)
    monkeypatch.setattr(ops, "conv2d_nhwc", rec_conv)
    monkeypatch.setattr(ops, "conv2d_wgrad_nhwc", rec_wgrad)
    net, cfg, _ = _build(train=True)
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    x0, eps, t = synth_inputs(4, 3, S, seed=5)
    loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
    loss.backward()
    n_train = (len(tile), len(tile_wgrad))
    net.eval()
    with torch.no_grad():
        net(torch.randn(4, 6, S, S, device=DEV), torch.rand(4, device=DEV) * 0.9 + 0.05)
    torch.cuda.synchronize()

    def limb(ci, co, k, stride):
        return k == 3 and stride == 1 and ci % 32 == 0 and co % 32 == 0 and ci >= 128 and co >= 128
    print("tile engine:", sorted(set(tile)), "wgrad:", sorted(set(tile_wgrad)), "train calls:", n_train)
    assert not [c for c in tile if limb(*c[:4])], tile
    assert not [c for c in tile_wgrad if limb(*c[:4])], tile_wgrad


def test_cli_afhqv2_128_inpaint_twice(tmp_path):
    """``inpaint --config afhqv2_128_inpaint`` on synthetic images with the synthetic mask, 3 EM steps, 2 images, from a
    checkpoint of synthetic weights, twice: uint8 [2, 128, 128, 3], identical."""
    from psld_amd import cli
    meta = _meta()
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    ck = str(tmp_path / "synth.ckpt")
    torch.save({"state_dict": {**{"score_fn." + k: v for k, v in sd.items()}, **{"ema_score_fn." + k: v for k, v in sd.items()}},
                "global_step": 0, "epoch": 0}, ck)
    outs = [str(tmp_path / "o1"), str(tmp_path / "o2")]
    for out in outs:
        cli.main(["inpaint", "--config", "afhqv2_128_inpaint", "--data", "synthetic", "--synthetic-size", "2", "--mask", "synthetic",
                  f"evaluation.chkpt_path={ck}", "evaluation.n_samples=2", "evaluation.batch_size=2", "evaluation.n_discrete_steps=3",
                  f"evaluation.save_path={out}", "evaluation.save_mode=np"])
    files = sorted(os.listdir(os.path.join(outs[0], "images")))
    assert files
    for f in files:
        a, b = np.load(os.path.join(outs[0], "images", f)), np.load(os.path.join(outs[1], "images", f))
        assert a.dtype == np.uint8 and a.shape == (2, 128, 128, 3)
        np.testing.assert_array_equal(a, b)
