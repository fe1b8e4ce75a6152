"""AFHQv2-128 on the GPU: the 3x3 limb kernels on 128x128 maps (Winograd F(2x2,3x3) 4 x 32 blocks, direct 2 x 64 blocks,
both weight-gradient forms) against fp64 torch, the full network against the reference's forward (net_afhq128.npz) and the
CPU oracle's gradients, where the executor sends the 128x128 level, and the command-line drivers with --config afhqv2_128."""
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
S = 128


# ---------------------------------------------------------------------------------------------------------------------
# kernels at 128x128
# ---------------------------------------------------------------------------------------------------------------------
FWD = [
    dict(b=1, c1=128, c2=0, co=128),
    dict(b=2, c1=128, c2=128, co=128),     # two sources: the up path's unmaterialised concatenation
    dict(b=1, c1=256, c2=0, co=128),
]


@pytest.mark.parametrize("form", ["wino", "direct", "direct_limb"])
@pytest.mark.parametrize("cfg", FWD)
def test_conv3x3_forward_128(ops, cfg, form):
    """Forward with the full epilogue (bias, time-embedding row bias, residual, scale) against fp64, repeatable bit for bit."""
    b, c1, c2, co = (cfg[n] for n in ("b", "c1", "c2", "co"))
    x = gen(b, c1 + c2, S, S, seed=40)
    w = gen(co, c1 + c2, 3, 3, seed=41, scale=0.05)
    bias, res, temb = gen(co, seed=42), gen(b, co, S, S, seed=43), gen(b, co, seed=44)
    ref = (F.conv2d(x.double(), w.double(), bias.double(), padding=1) + temb.double()[:, :, None, None] + res.double()) * 0.7
    x1 = _nhwc(x[:, :c1]).to(DEV)
    x2 = _nhwc(x[:, c1:]).to(DEV) if c2 else None
    epi = ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=S * S, residual=_nhwc(res).to(DEV),
                       ld_residual=co, out_scale=0.7)

    def run():
        y = torch.full((b, S, S, co), float("nan"), device=DEV)
        if form == "wino":
            assert ops.conv3x3_wino_supported(c1, c2, b, S, S, co)
            ops.conv3x3_wino(x1, x2, ops.conv3x3_wino_frag(w.to(DEV), False), co, y, epi)
        else:
            assert ops.conv3x3_split_supported(c1, c2, b, S, S, co)
            a1, a2 = x1, x2
            if form == "direct_limb":
                a1 = ops.f32_to_limb(x1)
                a2 = ops.f32_to_limb(x2) if c2 else None
            ops.conv3x3_split(a1, a2, ops.conv3x3_frag(w.to(DEV), False), co, y, epi)
        return y
    y = run()
    err = rel_l2(y.permute(0, 3, 1, 2), ref)
    print(f"{form} {cfg}: rel-L2 {err:.2e}")
    assert err < 3e-6
    assert torch.equal(y, run())


@pytest.mark.parametrize("form", ["wino", "direct"])
@pytest.mark.parametrize("ci,co", [(128, 128), (128, 256)])
def test_conv3x3_dgrad_128(ops, form, ci, co):
    """Data gradient (rotated, role-swapped filter) with the backward tape's alpha / accumulate epilogue."""
    b = 1
    x = gen(b, ci, S, S, seed=60).requires_grad_(True)
    w = gen(co, ci, 3, 3, seed=61, scale=0.05).requires_grad_(True)
    y = F.conv2d(x.double(), w.double(), padding=1)
    gy = gen(*y.shape, seed=62)
    y.backward(gy.double())
    gyd = _nhwc(gy).to(DEV)
    if form == "wino":
        frag, conv = ops.conv3x3_wino_frag(w.detach().to(DEV), True), ops.conv3x3_wino
    else:
        frag, conv = ops.conv3x3_frag(w.detach().to(DEV), True), ops.conv3x3_split
    dx = torch.full((b, S, S, ci), float("nan"), device=DEV)
    conv(gyd, None, frag, ci, dx)
    assert rel_l2(dx.permute(0, 3, 1, 2), x.grad) < 3e-6
    prev = gen(b, S, S, ci, seed=63).to(DEV)
    acc = prev.clone()
    conv(gyd, None, frag, ci, acc, ops.epilogue(alpha=0.5, accumulate=True))
    assert rel_l2(acc.permute(0, 3, 1, 2), 0.5 * x.grad + prev.permute(0, 3, 1, 2).cpu().double()) < 3e-6


@pytest.mark.parametrize("form", ["wino", "direct"])
@pytest.mark.parametrize("b,co", [(1, 128), (2, 256)])
def test_gn_partials_at_128(ops, form, b, co):
    """GroupNorm partial sums from the epilogue (one per 64-pixel run of a 4 x 32 / 2 x 64 block) against fp64 statistics
    of the written tensor."""
    c = 128
    x = gen(b, S, S, c, seed=70).to(DEV)
    w = gen(co, c, 3, 3, seed=71, scale=0.05).to(DEV)
    bias = gen(co, seed=72).to(DEV)
    part = ops.gn_part_buffer(b, S * S, co, DEV)
    part.fill_(float("nan"))
    y = torch.empty(b, S, S, co, device=DEV)
    epi = ops.epilogue(bias=bias, gn_part=part, gn_hw=S * S)
    if form == "wino":
        ops.conv3x3_wino(x, None, ops.conv3x3_wino_frag(w, False), co, y, epi)
    else:
        ops.conv3x3_split(x, None, ops.conv3x3_frag(w, False), co, y, epi)
    assert bool(torch.isfinite(part).all())
    gamma, beta = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)
    yd = y.double().cpu().reshape(b, S * S, co)
    for groups in (co // part.fine_width, co // 16):
        st = ops.gn_stats_from_part(part, y.shape, gamma, beta, groups=groups)
        g = yd.reshape(b, S * S, groups, co // groups)
        mean = g.mean(dim=(1, 3))
        var = g.var(dim=(1, 3), unbiased=False)
        assert rel_l2(st.mean, mean) < 1e-5 and rel_l2(st.rstd, (var + 1e-6).rsqrt()) < 1e-5


def test_conv3x3_wino_split_chunks_at_b1(ops):
    """The split-chunk form (small grids: B=1 at 256 -> 128 channels, 128 workgroups) against fp64, with accumulate,
    repeatable."""
    b, c1, co = 1, 256, 128
    if not ops.conv3x3_wino_ws_bytes(c1, 0, b, S, S, co):
        pytest.skip("this device's CU count fills the grid without a split")
    x = gen(b, c1, S, S, seed=40)
    w = gen(co, c1, 3, 3, seed=41, scale=0.05)
    bias, res = gen(co, seed=42), gen(b, co, S, S, seed=43)
    ref = (F.conv2d(x.double(), w.double(), bias.double(), padding=1) + res.double()) * 0.7
    x1 = _nhwc(x).to(DEV)
    uf = ops.conv3x3_wino_frag(w.to(DEV), False)
    epi = ops.epilogue(bias=bias.to(DEV), residual=_nhwc(res).to(DEV), ld_residual=co, out_scale=0.7)
    y1 = torch.full((b, S, S, co), float("nan"), device=DEV)
    ops.conv3x3_wino(x1, None, uf, co, y1, epi, allow_split=True)
    assert rel_l2(y1.permute(0, 3, 1, 2), ref) < 3e-6
    y2 = torch.full_like(y1, float("nan"))
    ops.conv3x3_wino(x1, None, uf, co, y2, epi, allow_split=True)
    assert torch.equal(y1, y2)
    acc = torch.ones_like(y1)
    ops.conv3x3_wino(x1, None, uf, co, acc, ops.epilogue(alpha=0.5, accumulate=True), allow_split=True)
    assert rel_l2(acc.permute(0, 3, 1, 2), F.conv2d(x.double(), w.double(), padding=1) * 0.5 + 1.0) < 3e-6


@pytest.mark.parametrize("c1,c2", [(128, 0), (128, 128)])
def test_conv3x3_wino_fused_groupnorm_128(ops, c1, c2):
    """GroupNorm + SiLU inside the Winograd staging == apply pass + convolution bit for bit, and fp64 within 5e-6."""
    b, co = 1, 128
    x = gen(b, c1 + c2, S, S, seed=70) * 1.5 + 0.3
    w = gen(co, c1 + c2, 3, 3, seed=71, scale=0.05)
    bias = gen(co, seed=72)
    x1 = _nhwc(x[:, :c1]).to(DEV)
    x2 = _nhwc(x[:, c1:]).to(DEV) if c2 else None
    g1, b1 = (gen(c1, seed=74) * 0.2 + 1.0).to(DEV), (gen(c1, seed=75) * 0.1).to(DEV)
    st1 = ops.gn_stats(x1, g1, b1)
    st2 = None
    if c2:
        g2, b2 = (gen(c2, seed=76) * 0.2 + 1.0).to(DEV), (gen(c2, seed=77) * 0.1).to(DEV)
        st2 = ops.gn_stats(x2, g2, b2)
    assert ops.conv3x3_wino_gn_supported(c1, c2, b, S, S, co)
    uf = ops.conv3x3_wino_frag(w.to(DEV), False)
    epi = ops.epilogue(bias=bias.to(DEV))
    y_ref = torch.full((b, S, S, co), float("nan"), device=DEV)
    ops.conv3x3_wino(ops.gn_apply(x1, st1, True), ops.gn_apply(x2, st2, True) if c2 else None, uf, co, y_ref, epi)
    y = torch.full_like(y_ref, float("nan"))
    ops.conv3x3_wino_gn(x1, st1, x2, st2, True, uf, co, y, epi)
    assert torch.equal(y, y_ref)

    def gn64(t, gamma, beta):
        return F.silu(F.group_norm(t.double(), ops.gn_groups(t.shape[1]), gamma.double().cpu(), beta.double().cpu(), eps=1e-6))
    parts = [gn64(x[:, :c1], g1, b1)] + ([gn64(x[:, c1:], g2, b2)] if c2 else [])
    ref = F.conv2d(torch.cat(parts, 1), w.double(), bias.double(), padding=1)
    assert rel_l2(y.permute(0, 3, 1, 2), ref) < 5e-6


def _wgrad_ref(b, ci1, ci2, co, seed):
    x = gen(b, ci1 + ci2, S, S, seed=seed)
    gy = gen(b, co, S, S, seed=seed + 1)
    xr = x.double().requires_grad_(True)
    w = torch.zeros(co, ci1 + ci2, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w, padding=1).backward(gy.double())
    return x, gy, w.grad


@pytest.mark.parametrize("b,ci1,ci2,co", [(1, 128, 0, 128), (2, 128, 128, 128), (1, 128, 0, 256)])
def test_conv3x3_wgrad_winograd_domain_128(ops, b, ci1, ci2, co):
    """Winograd-domain weight gradient (a K tile = half a tile row at W = 128): fp64 within 3e-6, two sources, accumulate,
    more than one K split, repeatable."""
    x, gy, ref = _wgrad_ref(b, ci1, ci2, co, 80)
    assert ops.conv3x3_wgrad_wino_supported(co, ci1, ci2, b, S, S)
    x1 = _nhwc(x[:, :ci1]).to(DEV)
    x2 = _nhwc(x[:, ci1:]).to(DEV) if ci2 else None
    dyd = _nhwc(gy).to(DEV)
    for ns in (None, 3):
        dw = torch.full((co, ci1 + ci2, 3, 3), float("nan"), device=DEV)
        ops.conv3x3_wgrad_wino(dyd, co, x1, dw, x2=x2, nsplit=ns)
        assert rel_l2(dw, ref) < 3e-6, ns
        dw2 = torch.full_like(dw, float("nan"))
        ops.conv3x3_wgrad_wino(dyd, co, x1, dw2, x2=x2, nsplit=ns)
        assert torch.equal(dw, dw2)
    prev = gen(co, ci1 + ci2, 3, 3, seed=89).to(DEV)
    acc = prev.clone()
    ops.conv3x3_wgrad_wino(dyd, co, x1, acc, x2=x2, accumulate=True, alpha=0.5)
    assert rel_l2(acc, 0.5 * ref + prev.cpu().double()) < 3e-6


@pytest.mark.parametrize("limb", [False, True])
@pytest.mark.parametrize("b,ci1,ci2,co", [(1, 128, 0, 128), (2, 128, 128, 128), (1, 128, 0, 64)])
def test_conv3x3_wgrad_direct_128(ops, limb, b, ci1, ci2, co):
    """Direct limb weight gradient (32-pixel K tiles at column offsets 0 / 32 / 64 / 96): fp64 within 3e-6, two sources,
    x as fp32 or as limb planes, K split as the executor splits it, repeatable."""
    x, gy, ref = _wgrad_ref(b, ci1, ci2, co, 90)
    assert ops.conv3x3_wgrad_split_supported(co, ci1, b, S, S)
    x1 = _nhwc(x[:, :ci1]).to(DEV)
    x2 = _nhwc(x[:, ci1:]).to(DEV) if ci2 else None
    if limb:
        x1 = ops.f32_to_limb(x1)
        x2 = ops.f32_to_limb(x2) if ci2 else None
    dyd = _nhwc(gy).to(DEV)
    cin = ci1 + ci2
    outs = []
    for ns in (4, 16, 16):
        slabs = torch.full((ns, co, 9, cin), float("nan"), device=DEV)
        ops.conv3x3_wgrad_split(dyd, co, x1, slabs, cin, 0, ns, x2)
        dw = slabs.double().sum(0).reshape(co, 3, 3, cin).permute(0, 3, 1, 2)
        assert rel_l2(dw, ref) < 3e-6, ns
        outs.append(slabs)
    assert torch.equal(outs[1], outs[2])


# ---------------------------------------------------------------------------------------------------------------------
# the AFHQv2-128 network
# ---------------------------------------------------------------------------------------------------------------------
def _build(train=False, dropout=None):
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    import json
    from tests.conftest import GOLDEN
    with open(os.path.join(GOLDEN, "afhq_meta.json")) as fh:
        meta = json.load(fh)
    cfg = C.afhqv2_128()
    if dropout is not None:
        cfg.model.score_fn.dropout = dropout
    net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    net.train(train)
    return net, cfg, sd


@pytest.mark.parametrize("mode", ["wino1", "wino2", "wino0", "f32"])
def test_afhq128_forward_matches_reference(golden, mode):
    from psld_amd import ops
    net, cfg, _ = _build()
    g = golden("net_afhq128.npz")
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
    print(f"afhq128 {mode}: rel-L2 vs reference = {err:.3e}")
    assert y.shape == g["y"].shape and err < 2e-5


@pytest.mark.parametrize("winograd,wgrad", [(1, 1), (2, 2), (0, 0)])
def test_afhq128_gradients_against_live_oracle(winograd, wgrad):
    """Every parameter gradient of the 65.8 M-parameter network vs torch autograd through the oracle on the CPU (B = 1,
    dropout 0): the gates of test_full_size_network_gradients_against_live_oracle."""
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
    print(f"afhq128 ({winograd},{wgrad}): global grad rel-L2 {np.sqrt(num / den):.3e}; worst {worst:.3e} ({worst_k})")
    assert np.sqrt(num / den) < 2e-5
    assert worst < 1e-4, (worst, worst_k)


def test_afhq128_dispatch_keeps_limb_shapes_off_the_tile_engine(monkeypatch):
    """One training step and one eval forward at B = 8: no 3x3 stride-1 convolution with channels the limb kernels take
    (multiples of 32 in, of 128 out) reaches the fp32 tile engine - forward, data gradient or weight gradient - at any map
    size, and the GroupNorms of the 128x128 level take their statistics from epilogue partial sums.  Three statistics passes
    remain there, none behind a limb-kernel convolution: two over the stem's output (a 6-channel convolution - as the first
    block's input, and as one source of the up path's last concatenation) and one over the up path's first concatenation,
    256 + 128 channels, whose 12-channel groups straddle the two sources (it is materialised for its GroupNorm)."""
    from psld_amd import ops
    from psld_amd.registry import get_module
    tile, tile_wgrad, stats = [], [], []
    conv, wgrad, gn_stats = ops.conv2d_nhwc, ops.conv2d_wgrad_nhwc, ops.gn_stats

    def rec_conv(x1, x2, w_ohwi, cout, kh, kw, stride, pad, *a, **k):
        tile.append((x1.shape[-1] + (x2.shape[-1] if x2 is not None else 0), cout, kh, stride, x1.shape[2]))
        return conv(x1, x2, w_ohwi, cout, kh, kw, stride, pad, *a, **k)

    def rec_wgrad(dy, cout, x, kh, kw, stride, *a, **k):
        tile_wgrad.append((x.shape[-1], cout, kh, stride, x.shape[2]))
        return wgrad(dy, cout, x, kh, kw, stride, *a, **k)

    def rec_stats(x, *a, **k):
        stats.append(tuple(x.shape))
        return gn_stats(x, *a, **k)
    monkeypatch.setattr(ops, "conv2d_nhwc", rec_conv)
    monkeypatch.setattr(ops, "conv2d_wgrad_nhwc", rec_wgrad)
    monkeypatch.setattr(ops, "gn_stats", rec_stats)
    net, cfg, _ = _build(train=True)
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    x0, eps, t = synth_inputs(8, 3, S, seed=5)
    loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
    loss.backward()
    train_stats = [s for s in stats if s[1] == S]
    stats.clear()
    net.eval()
    with torch.no_grad():
        net(torch.randn(8, 6, S, S, device=DEV), torch.rand(8, device=DEV) * 0.9 + 0.05)
    eval_stats = [s for s in stats if s[1] == S]
    torch.cuda.synchronize()

    def limb(ci, co, k, stride):
        return k == 3 and stride == 1 and ci % 32 == 0 and co % 128 == 0
    print("tile engine:", sorted(set(tile)), "wgrad:", sorted(set(tile_wgrad)))
    print("128x128 statistics passes: train", train_stats, "eval", eval_stats)
    assert not [c for c in tile if limb(*c[:4])], tile
    assert not [c for c in tile_wgrad if limb(*c[:4])], tile_wgrad
    expected = [(8, S, S, 128), (8, S, S, 128), (8, S, S, 384)]
    assert sorted(train_stats) == expected and sorted(eval_stats) == expected, (train_stats, eval_stats)


def test_cli_afhqv2_128_train_checkpoint_sample(tmp_path):
    """The drivers with --config afhqv2_128: 2 training steps on 16 synthetic images, a checkpoint, then 2 images with 3 EM
    steps, twice: uint8 [2, 128, 128, 3], identical."""
    from psld_amd import cli
    res, out1, out2 = str(tmp_path / "run"), str(tmp_path / "s1"), str(tmp_path / "s2")
    common = ["--config", "afhqv2_128"]
    cli.main(["train", *common, "--max-steps", "2", "--synthetic-size", "16", "--log-every", "1",
              "dataset.diffusion.training.batch_size=8", "dataset.diffusion.training.epochs=1",
              f"dataset.diffusion.training.results_dir='{res}'", "training.chkpt_prefix=t"])
    ck = os.path.join(res, "checkpoints", "last.ckpt")
    sd = torch.load(ck, map_location="cpu", weights_only=False)
    assert sd["global_step"] == 2
    for out in (out1, out2):
        cli.main(["sample", *common, f"evaluation.chkpt_path={ck}", "evaluation.n_samples=2", "evaluation.batch_size=2",
                  "evaluation.n_discrete_steps=3", f"evaluation.save_path={out}", "evaluation.save_mode=np",
                  "evaluation.sample_prefix=gpu"])
    files = sorted(os.listdir(os.path.join(out1, "images")))
    assert files
    for f in files:
        a, b = np.load(os.path.join(out1, "images", f)), np.load(os.path.join(out2, "images", f))
        assert a.dtype == np.uint8 and a.shape == (2, 128, 128, 3)
        np.testing.assert_array_equal(a, b)
