"""Math mode 'bf16x3' on the GPU: the two-limb packers, Winograd forward and pointwise forward kernels against the CPU
reference of the arithmetic (tests/x3_ref.py, fp64 accumulation: the kernels differ from it in fp32 summation order only,
the project's 3e-6 kernel gate), the networks and samplers under the mode against the reference goldens (the 1e-4 parity
contract), what the executor dispatches, and the CLI option.  Every test restores the process's math mode."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from psld_amd import config as C
from tests import x3_ref as X
from tests.synth import synth_inputs, synth_state_dict
from tests.test_kernels_gpu import _nhwc, gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.from_numpy


@contextlib.contextmanager
def math(mode, winograd=None, fused_gn=None):
    from psld_amd import ops as o
    old = o.math_mode()
    try:
        o.set_math_mode(mode)
        o.set_winograd(winograd)
        o.set_fused_gn(fused_gn)
        yield
    finally:
        o.set_winograd(None)
        o.set_fused_gn(None)
        o.set_math_mode(old)


# ---------------------------------------------------------------------------------------------------------------------
# packers
# ---------------------------------------------------------------------------------------------------------------------
def _planes(buf, limbs, payload):
    """[blocks][limbs][64 lanes x 16 bytes] view of a fragment buffer's payload."""
    return buf[:payload].view(torch.int32).reshape(-1, limbs, 256)


@pytest.mark.parametrize("co,ci", [(128, 128), (256, 512), (160, 320)])
def test_wino_packer_planes(ops, co, ci):
    """The two planes of a two-limb Winograd fragment buffer are the hi and mid planes of the three-limb buffer, bit for
    bit; the batched refresh writes what the single launch writes."""
    w = gen(co, ci, 3, 3, seed=11, scale=0.05).to(DEV)
    w2 = gen(co, ci, 3, 3, seed=12, scale=0.05).to(DEV)
    f3, f2 = ops.conv3x3_wino_frag(w, False), ops.conv3x3_wino_frag_x3(w)
    assert f2.numel() == ops.conv3x3_wino_frag_bytes_x3(co, ci) == co * ci * 64 + 16384
    p3, p2 = _planes(f3, 3, co * ci * 96), _planes(f2, 2, co * ci * 64)
    assert torch.equal(p2, p3[:, :2])
    outs = [torch.zeros_like(f2), torch.zeros_like(f2)]
    rows, total = [], 0
    for wt, out in zip((w, w2), outs):
        rows.append(ops.conv3x3_wino_frag_entry(wt, False, out) + [total])
        total += co * ci // 8
    ops.pack_wino_batch_x3(torch.tensor(rows, dtype=torch.int64, device=DEV), 2, total)
    assert torch.equal(outs[0][:co * ci * 64], f2[:co * ci * 64])
    assert torch.equal(outs[1][:co * ci * 64], ops.conv3x3_wino_frag_x3(w2)[:co * ci * 64])


@pytest.mark.parametrize("n,k", [(256, 256), (256, 512), (768, 256)])
def test_gemm_packer_planes(ops, n, k):
    b = gen(k, n, seed=13, scale=0.05).to(DEV)              # a [k][n] matrix (NIN.W): stride_n = 1, stride_k = n
    f3, f2 = ops.gemm_frag(b, n, k, 1, n), ops.gemm_frag_x3(b, n, k, 1, n)
    assert f2.numel() == ops.gemm_frag_bytes_x3(n, k) == n * k * 4
    assert torch.equal(_planes(f2, 2, n * k * 4), _planes(f3, 3, n * k * 6)[:, :2])
    out = torch.zeros_like(f2)
    row = [b.data_ptr(), out.data_ptr(), n, k, 1, 1, n, 0]
    ops.pack_frag_batch_x3(torch.tensor([row], dtype=torch.int64, device=DEV), 1, n * k // 8)
    assert torch.equal(out, f2)


# ---------------------------------------------------------------------------------------------------------------------
# Winograd forward, two limbs
# ---------------------------------------------------------------------------------------------------------------------
WINO = [
    dict(b=8, c1=128, c2=0, co=128, s=32),
    dict(b=8, c1=256, c2=0, co=256, s=32),
    dict(b=8, c1=256, c2=0, co=256, s=16),
    dict(b=8, c1=256, c2=0, co=256, s=8),
    dict(b=8, c1=256, c2=128, co=256, s=16),       # two sources
    dict(b=2, c1=128, c2=0, co=128, s=64),
    dict(b=1, c1=128, c2=0, co=128, s=128),
    dict(b=2, c1=160, c2=0, co=160, s=32),         # channel tails
    dict(b=2, c1=320, c2=0, co=480, s=16),
    dict(b=1, c1=256, c2=0, co=256, s=16, split=True),      # split-chunk form
]


@pytest.mark.parametrize("cfg", WINO, ids=lambda c: "{b}x{c1}+{c2}->{co}@{s}".format(**c))
def test_conv3x3_wino_x3_forward(ops, cfg):
    """Full epilogue (bias, time-embedding row bias, residual, scale), alpha + accumulate, GroupNorm partial sums and the
    fused GroupNorm + SiLU staging, each against the two-limb reference within 3e-6 and repeated bit for bit.  Against a
    true fp64 convolution the kernel is no worse than twice the reference's own error - and more than 1e-6 away: a silent
    fall-back to three limbs would show."""
    b, c1, c2, co, s = (cfg[n] for n in ("b", "c1", "c2", "co", "s"))
    split = cfg.get("split", False)
    assert ops.conv3x3_wino_supported(c1, c2, b, s, s, co)
    if split and not ops.conv3x3_wino_ws_bytes(c1, c2, b, s, s, co):
        pytest.skip("this device's CU count fills the grid without a split")
    x = gen(b, c1 + c2, s, s, seed=40)
    w = gen(co, c1 + c2, 3, 3, seed=41, scale=0.05)
    bias, res, temb = gen(co, seed=42), gen(b, co, s, s, seed=43), gen(b, co, seed=44)
    conv_emu = X.two_limb_conv3x3(x, w)
    conv64 = F.conv2d(x.double(), w.double(), padding=1)
    x1 = _nhwc(x[:, :c1]).to(DEV)
    x2 = _nhwc(x[:, c1:]).to(DEV) if c2 else None
    uf = ops.conv3x3_wino_frag_x3(w.to(DEV))
    tag = "{b}x{c1}+{c2}->{co}@{s}".format(**cfg)

    def run(e, init):
        y = init.clone()
        ops.conv3x3_wino_x3(x1, x2, uf, co, y, e, allow_split=split)
        return y
    nan = torch.full((b, s, s, co), float("nan"), device=DEV)
    # plain: the arithmetic itself
    y = run(None, nan)
    e_emu, e_64, emu_64 = rel_l2(y.permute(0, 3, 1, 2), conv_emu), rel_l2(y.permute(0, 3, 1, 2), conv64), rel_l2(conv_emu, conv64)
    print(f"wino x3 {tag}: vs two-limb reference {e_emu:.2e}, vs fp64 {e_64:.2e} (reference vs fp64 {emu_64:.2e})")
    assert e_emu <= 3e-6
    assert 1e-6 < e_64 <= 2 * emu_64
    assert torch.equal(y, run(None, nan))
    # full epilogue
    epi = ops.epilogue(bias=bias.to(DEV), rowbias=temb.to(DEV), rows_per_img=s * s, residual=_nhwc(res).to(DEV),
                       ld_residual=co, out_scale=0.7)
    ref = (conv_emu + bias.double()[None, :, None, None] + temb.double()[:, :, None, None] + res.double()) * 0.7
    y = run(epi, nan)
    err = rel_l2(y.permute(0, 3, 1, 2), ref)
    print(f"wino x3 {tag} full epilogue: {err:.2e}")
    assert err <= 3e-6 and torch.equal(y, run(epi, nan))
    # alpha + accumulate
    prev = gen(b, s, s, co, seed=49).to(DEV)
    acc = run(ops.epilogue(alpha=0.5, accumulate=True), prev)
    err = rel_l2(acc.permute(0, 3, 1, 2), conv_emu * 0.5 + prev.permute(0, 3, 1, 2).cpu().double())
    print(f"wino x3 {tag} accumulate: {err:.2e}")
    assert err <= 3e-6 and torch.equal(acc, run(ops.epilogue(alpha=0.5, accumulate=True), prev))
    # GroupNorm partial sums of the output (whole 128-channel tiles only)
    if co % 128 == 0 and ops.gn_part_supported(b, s * s, co):
        part = ops.gn_part_buffer(b, s * s, co, DEV)
        part.fill_(float("nan"))
        y = run(ops.epilogue(bias=bias.to(DEV), gn_part=part, gn_hw=s * s), nan)
        assert bool(torch.isfinite(part).all())
        assert rel_l2(y.permute(0, 3, 1, 2), conv_emu + bias.double()[None, :, None, None]) <= 3e-6
        groups = co // 16
        st = ops.gn_stats_from_part(part, y.shape, torch.ones(co, device=DEV), torch.zeros(co, device=DEV), groups=groups)
        g = y.double().cpu().reshape(b, s * s, groups, co // groups)
        assert rel_l2(st.mean, g.mean(dim=(1, 3))) < 1e-5
        assert rel_l2(st.rstd, (g.var(dim=(1, 3), unbiased=False) + 1e-6).rsqrt()) < 1e-5
    # GroupNorm + SiLU inside the staging: bit for bit the apply pass + the convolution, and the reference on the same input
    if ops.conv3x3_wino_gn_supported(c1, c2, b, s, s, co):
        xs = x * 1.5 + 0.3
        xs1 = _nhwc(xs[:, :c1]).to(DEV)
        xs2 = _nhwc(xs[:, c1:]).to(DEV) if c2 else None
        st1 = ops.gn_stats(xs1, (gen(c1, seed=74) * 0.2 + 1.0).to(DEV), (gen(c1, seed=75) * 0.1).to(DEV))
        st2 = ops.gn_stats(xs2, (gen(c2, seed=76) * 0.2 + 1.0).to(DEV), (gen(c2, seed=77) * 0.1).to(DEV)) if c2 else None
        a1 = ops.gn_apply(xs1, st1, True)
        a2 = ops.gn_apply(xs2, st2, True) if c2 else None
        e = ops.epilogue(bias=bias.to(DEV))
        y_un = nan.clone()
        ops.conv3x3_wino_x3(a1, a2, uf, co, y_un, e, allow_split=split)
        y_f = nan.clone()
        ops.conv3x3_wino_gn_x3(xs1, st1, xs2, st2, True, uf, co, y_f, e, allow_split=split)
        assert torch.equal(y_f, y_un)
        y_f2 = nan.clone()
        ops.conv3x3_wino_gn_x3(xs1, st1, xs2, st2, True, uf, co, y_f2, e, allow_split=split)
        assert torch.equal(y_f, y_f2)
        act = torch.cat([a1] + ([a2] if c2 else []), -1).permute(0, 3, 1, 2).cpu()
        err = rel_l2(y_f.permute(0, 3, 1, 2), X.two_limb_conv3x3(act, w) + bias.double()[None, :, None, None])
        print(f"wino x3 {tag} fused GroupNorm + SiLU: {err:.2e}")
        assert err <= 3e-6


# ---------------------------------------------------------------------------------------------------------------------
# pointwise forward, two limbs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k1,k2,n", [(256, 0, 256), (512, 0, 256), (256, 256, 256), (256, 0, 768)])
def test_gemm_split_x3_forward(ops, k1, k2, n):
    """M = 8 x 32 x 32 rows.  psld_gemm_split_supported takes no 160-wide case (n must be a multiple of 128), so there is
    none here."""
    m = 8 * 32 * 32
    assert ops.gemm_split_x3_supported(k1, k2, m, n)
    assert not ops.gemm_split_supported(160, 0, m, 160)
    a = gen(m, k1 + k2, seed=50)
    bm = gen(n, k1 + k2, seed=51, scale=0.05)               # [n][k]
    bias, res = gen(n, seed=52), gen(m, n, seed=53)
    emu, ref64 = X.two_limb_matmul(a, bm), a.double() @ bm.double().t()
    a1 = a[:, :k1].contiguous().to(DEV)
    a2 = a[:, k1:].contiguous().to(DEV) if k2 else None
    fr = ops.gemm_frag_x3(bm.to(DEV), n, k1 + k2, k1 + k2, 1)

    def run(e, init):
        y = init.clone()
        ops.gemm_split_x3(a1, a2, m, fr, n, y, e)
        return y
    nan = torch.full((m, n), float("nan"), device=DEV)
    y = run(None, nan)
    e_emu, e_64, emu_64 = rel_l2(y, emu), rel_l2(y, ref64), rel_l2(emu, ref64)
    print(f"gemm x3 {k1}+{k2}->{n} m={m}: vs two-limb reference {e_emu:.2e}, vs fp64 {e_64:.2e} (reference vs fp64 {emu_64:.2e})")
    assert e_emu <= 3e-6
    assert 1e-6 < e_64 <= 2 * emu_64
    assert torch.equal(y, run(None, nan))
    epi = ops.epilogue(bias=bias.to(DEV), residual=res.to(DEV), ld_residual=n, out_scale=0.7)
    y = run(epi, nan)
    assert rel_l2(y, (emu + bias.double() + res.double()) * 0.7) <= 3e-6 and torch.equal(y, run(epi, nan))
    prev = gen(m, n, seed=54).to(DEV)
    acc = run(ops.epilogue(alpha=0.5, accumulate=True), prev)
    assert rel_l2(acc, emu * 0.5 + prev.cpu().double()) <= 3e-6
    assert torch.equal(acc, run(ops.epilogue(alpha=0.5, accumulate=True), prev))
    hw = 1024
    if ops.gn_part_supported(m // hw, hw, n):
        part = ops.gn_part_buffer(m // hw, hw, n, DEV)
        part.fill_(float("nan"))
        y = run(ops.epilogue(bias=bias.to(DEV), gn_part=part, gn_hw=hw), nan)
        assert bool(torch.isfinite(part).all()) and rel_l2(y, emu + bias.double()) <= 3e-6
        groups = ops.gn_groups(n)
        st = ops.gn_stats_from_part(part, (m // hw, 32, 32, n), torch.ones(n, device=DEV), torch.zeros(n, device=DEV),
                                    groups=groups)
        g = y.double().cpu().reshape(m // hw, hw, groups, n // groups)
        assert rel_l2(st.mean, g.mean(dim=(1, 3))) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------------------
LIMB3 = ("conv3x3_wino", "conv3x3_wino_gn", "gemm_split")
LIMB2 = ("conv3x3_wino_x3", "conv3x3_wino_gn_x3", "gemm_split_x3")


def _record(monkeypatch, log, phase=lambda: None):
    """Recording wrappers around the limb entry points of ``ops``: (name, phase, x3 would take the shape)."""
    from psld_amd import ops as o
    for name in LIMB3 + LIMB2:
        fn = getattr(o, name)

        def rec(*a, _fn=fn, _name=name, **k):
            takes = True
            if _name == "gemm_split":
                a1, a2, m, n = a[0], a[1], a[2], a[4]
                takes = o.gemm_split_x3_wanted(a1.shape[-1], a2.shape[-1] if a2 is not None else 0, m, n)
            log.append((_name, phase(), takes))
            return _fn(*a, **k)
        monkeypatch.setattr(o, name, rec)


def _net(name):
    if name in ("c10_sota", "celeba64"):
        from tests.test_model_gpu import _build
        return _build(name)[0], f"net_{name}.npz"
    if name == "afhqv2_128":
        from tests.test_afhq_gpu import _build
        return _build()[0], "net_afhq128.npz"
    from tests.test_afhq160_gpu import _build
    return _build()[0], "net_afhq160.npz"


@pytest.mark.parametrize("name", ["c10_sota", "celeba64", "afhqv2_128", "afhqv2_128_inpaint"])
def test_network_forward_under_bf16x3(golden, monkeypatch, name):
    """Eval forward against the reference golden under 'bf16x3' with every supported 3x3 convolution on the two-limb
    Winograd kernel (the goldens' batches are below the default policy's thresholds); 'bf16x6' before and after the visit is
    bitwise the same (separate cache entries); no three-limb Winograd-forward / pointwise launch where a two-limb one exists."""
    net, gname = _net(name)
    g = golden(gname)
    x, t = T(g["x"]).to(DEV), T(g["t"]).to(DEV)
    log = []
    with math("bf16x6", winograd=2, fused_gn=2), torch.no_grad():
        y6 = net(x, t)
    _record(monkeypatch, log)
    with math("bf16x3", winograd=2, fused_gn=2), torch.no_grad():
        y3 = net(x, t)
        y3b = net(x, t)
    monkeypatch.undo()
    with math("bf16x6", winograd=2, fused_gn=2), torch.no_grad():
        y6b = net(x, t)
    e3, e6, d = rel_l2(y3, T(g["y"])), rel_l2(y6, T(g["y"])), rel_l2(y3, y6)
    print(f"{name}: bf16x3 {e3:.3e}, bf16x6 {e6:.3e} vs the reference golden; bf16x3 vs bf16x6 {d:.3e}")
    assert e3 < 1e-4
    assert torch.equal(y6, y6b) and torch.equal(y3, y3b)
    assert not torch.equal(y3, y6) and d < 1e-4
    names = [n for n, _, _ in log]
    assert "conv3x3_wino_x3" in names or "conv3x3_wino_gn_x3" in names
    assert not [r for r in log if r[0] in ("conv3x3_wino", "conv3x3_wino_gn")], sorted(set(names))
    assert not [r for r in log if r[0] == "gemm_split" and r[2]]


def test_pointwise_dispatch_and_batch_rows_at_b16(monkeypatch, golden):
    """C10-SOTA at B = 16 under the default policy: the 32x32 level's shortcut and attention projections (128 tiles and more)
    run the two-limb pointwise kernel, and rows [0:2] equal the B = 2 run to fp32 rounding."""
    from tests.test_model_gpu import _build
    net, _, _ = _build("c10_sota")
    g = golden("net_c10_sota.npz")
    x2, t2 = T(g["x"]).to(DEV), T(g["t"]).to(DEV)
    gg = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(16, 6, 32, 32, device=DEV, generator=gg)
    t = torch.rand(16, device=DEV, generator=gg) * 0.9 + 0.05
    x[:2], t[:2] = x2, t2
    log = []
    _record(monkeypatch, log)
    with math("bf16x3"), torch.no_grad():
        y16 = net(x, t)
        y2 = net(x2, t2)
    names = [n for n, _, _ in log]
    print("B=16 + B=2 launches:", {n: names.count(n) for n in set(names)})
    assert "gemm_split_x3" in names and ("conv3x3_wino_x3" in names or "conv3x3_wino_gn_x3" in names)
    assert not [r for r in log if r[0] in ("conv3x3_wino", "conv3x3_wino_gn")]
    assert not [r for r in log if r[0] == "gemm_split" and r[2]]
    assert rel_l2(y16[:2], T(g["y"])) < 1e-4 and rel_l2(y16[:2], y2) < 1e-4


def test_training_step_under_bf16x3_is_the_bf16x6_step(monkeypatch):
    """A recording pass runs 'bf16x6' launches whatever the mode says: none of the two-limb entry points is called, and
    loss, gradients and updated parameters are bitwise those of 'bf16x6'."""
    from psld_amd.optim import FusedAdam
    from psld_amd.registry import get_module
    from tests.test_model_gpu import _build
    res = {}
    log = []
    for mode in ("bf16x6", "bf16x3"):
        with math(mode):
            net, cfg, _ = _build("c10_sota", train=True)
            cfg.model.score_fn.dropout = 0.0
            sde = get_module("sde", "psld")(cfg)
            crit = get_module("losses", "psld_score_loss")(cfg, sde)
            x0, eps, t = synth_inputs(16, 3, 32, seed=5)
            if mode == "bf16x3":
                _record(monkeypatch, log)
            opt = FusedAdam(net, lr=1e-3, grad_clip=1.0)
            loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
            loss.backward()
            grads = [net.flat_grad().clone()]
            opt.step()
            res[mode] = (loss.detach().clone(), grads, [p.detach().clone() for p in net.parameters()])
            monkeypatch.undo()
    names = [n for n, _, _ in log]
    assert names and not [n for n in names if n in LIMB2], sorted(set(names))
    assert torch.equal(res["bf16x6"][0], res["bf16x3"][0])
    for a, b in zip(res["bf16x6"][1] + res["bf16x6"][2], res["bf16x3"][1] + res["bf16x3"][2]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", ["uniform", "quadratic"])
def test_em_sampler_under_bf16x3_matches_reference(golden, stride):
    from psld_amd.registry import get_module
    from tests.test_fullsize_gpu import _sampler
    from tests.test_model_gpu import _build
    net, cfg, _ = _build("c10_sota")
    g = golden("em_c10_sota.npz")
    noise = T(g[f"noise_{stride}"]).to(DEV)
    sde, sampler, _ = _sampler(cfg, net, noise)
    cfg.evaluation.n_discrete_steps = 4
    cfg.evaluation.stride_type = stride
    wr = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=net, sampler_cls=None)
    ts = wr.sampling_times(DEV)
    with math("bf16x3", winograd=2, fused_gn=2):
        x = sampler.sample(T(g[f"batch_{stride}"]).to(DEV), ts, wr.n_discrete_steps, denoise=True, eps=cfg.evaluation.eval_eps)
    err = rel_l2(x, T(g[f"x_{stride}"]))
    print(f"EM on C10-SOTA under bf16x3 ({stride}): rel-L2 vs reference = {err:.3e}")
    assert x.dtype == torch.float64 and err < 1e-4


def test_graph_replay_and_batch_independence_under_bf16x3(golden):
    """The graph-replayed eval forward equals the eager one bit for bit in the mode, a capture made under 'bf16x6' is not
    replayed under 'bf16x3', and the first 4 rows of a B = 8 EM run equal the B = 4 run."""
    from tests.test_fullsize_gpu import _sampler
    from tests.test_model_gpu import _build
    net, cfg, _ = _build("c10_sota")
    g = golden("em_c10_sota.npz")
    gg = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(8, 6, 32, 32, device=DEV, generator=gg)
    t = torch.rand(8, device=DEV, generator=gg) * 0.9 + 0.05
    with math("bf16x6", winograd=2, fused_gn=2), torch.no_grad():
        e6 = net(x, t)
        net.enable_graphs(True)
        g6 = net(x, t)
    try:
        with math("bf16x3", winograd=2, fused_gn=2), torch.no_grad():
            g3 = net(x, t)
            g3b = net(x, t)
            net.enable_graphs(False)
            e3 = net(x, t)
    finally:
        net.enable_graphs(False)
    assert torch.equal(e6, g6) and torch.equal(e3, g3) and torch.equal(g3, g3b) and not torch.equal(e3, e6)
    noise = torch.randn(2, 8, 6, 32, 32, device=DEV, generator=gg, dtype=torch.float64)
    batch = torch.randn(8, 6, 32, 32, device=DEV, generator=gg)
    ts = T(g["ts_uniform"]).to(DEV)[:3]
    with math("bf16x3", winograd=2, fused_gn=2):
        _, s8, _ = _sampler(cfg, net, noise)
        x8 = s8.sample(batch, ts, 2, denoise=True, eps=cfg.evaluation.eval_eps)
        _, s4, _ = _sampler(cfg, net, noise[:, :4])
        x4 = s4.sample(batch[:4], ts, 2, denoise=True, eps=cfg.evaluation.eval_eps)
    err = rel_l2(x8[:4], x4)
    print(f"bf16x3 EM, B=8 rows [0:4] vs B=4: {err:.3e}")
    assert err < 5e-6           # test_fullsize_gpu.py's bound for the same kernels on other tilings


def test_inpainting_sampler_under_bf16x3(monkeypatch):
    """3 ip_em_sde steps of afhqv2_128_inpaint at B = 2, synthetic weights, fixed draws: the 'bf16x3' state against the
    'bf16x6' state of the same run (the parent's code path) within the 1e-4 contract, on two-limb launches."""
    from psld_amd.registry import get_module
    from tests.test_afhq160_gpu import _build
    net, cfg, _ = _build()
    sde = get_module("sde", "psld")(cfg)
    gg = torch.Generator().manual_seed(3)
    x0 = torch.rand(2, 3, 128, 128, generator=gg) * 2 - 1
    mask = torch.ones(2, 3, 128, 128)
    mask[:, :, 32:96, 32:96] = 0
    ts = torch.linspace(0, 1.0 - cfg.evaluation.eval_eps, 4, dtype=torch.float64).to(DEV)
    out, log = {}, []
    for mode in ("bf16x6", "bf16x3"):
        sampler = get_module("samplers", "ip_em_sde")(cfg, sde, net)
        dg = torch.Generator().manual_seed(17)
        sampler.draw_fn = lambda shape, dtype, device: torch.randn(*shape, generator=dg, dtype=torch.float64).to(device=device, dtype=dtype)
        if mode == "bf16x3":
            _record(monkeypatch, log)
        with math(mode):
            out[mode] = sampler.sample((x0.to(DEV), mask.to(DEV)), ts, 3, denoise=True, eps=cfg.evaluation.eval_eps)
        monkeypatch.undo()
    err = rel_l2(out["bf16x3"], out["bf16x6"])
    names = [n for n, _, _ in log]
    print(f"ip_em_sde afhqv2_128_inpaint, 3 steps: bf16x3 vs bf16x6 {err:.3e}; launches {dict((n, names.count(n)) for n in set(names))}")
    assert 0 < err < 1e-4
    assert [n for n in names if n in LIMB2] and not [n for n in names if n in ("conv3x3_wino", "conv3x3_wino_gn")]


def test_class_conditional_sampler_under_bf16x3(monkeypatch):
    """3 cc_em_sde steps of C10-SOTA with the clf_c10 classifier at B = 16 (synthetic weights, fixed noise): 'bf16x3' against
    'bf16x6' within 1e-4; the score network runs two-limb launches, the classifier's recorded pass three-limb ones."""
    import psld_amd
    from psld_amd.registry import get_module
    from tests.test_model_gpu import _build
    psld_amd.import_modules_into_registry()
    net, dcfg, _ = _build("c10_sota")
    ccfg = C.clf_c10()
    clf = get_module("clf_fn", "ncsnpp_clf")(ccfg)
    clf.load_state_dict(synth_state_dict([(k, tuple(v.shape)) for k, v in clf.state_dict().items()], 23), strict=True)
    clf = clf.to(DEV).eval()
    root = C.with_clf(dcfg, ccfg)
    root.clf.evaluation.clf_temp = 1.0
    root.clf.evaluation.label_to_sample = 3
    sde = get_module("sde", "psld")(dcfg)
    gg = torch.Generator(device=DEV).manual_seed(31)
    B = 16
    batch = torch.randn(B, 6, 32, 32, device=DEV, generator=gg)
    noise = torch.randn(4, B, 6, 32, 32, device=DEV, generator=gg, dtype=torch.float64)
    ts = torch.linspace(0, 1.0 - dcfg.evaluation.eval_eps, 4, dtype=torch.float64).to(DEV)
    out, log = {}, []
    for mode in ("bf16x6", "bf16x3"):
        sampler = get_module("samplers", "cc_em_sde")(root, sde, net, clf)
        sampler.noise_fn = lambda i, x: noise[i]
        phase = ["score"]
        guidance = sampler._guidance

        def in_clf(x32, t, _g=guidance, _p=phase):
            _p[0] = "clf"
            try:
                return _g(x32, t)
            finally:
                _p[0] = "score"
        sampler._guidance = in_clf
        if mode == "bf16x3":
            _record(monkeypatch, log, lambda: phase[0])
        with math(mode):
            out[mode] = sampler.sample(batch, ts, 3, denoise=True, eps=dcfg.evaluation.eval_eps)
        monkeypatch.undo()
    err = rel_l2(out["bf16x3"], out["bf16x6"])
    print(f"cc_em_sde C10-SOTA + clf_c10, 3 steps: bf16x3 vs bf16x6 {err:.3e}")
    assert 0 < err < 1e-4
    score = [n for n, p, _ in log if p == "score"]
    clfl = [n for n, p, _ in log if p == "clf"]
    assert [n for n in score if n in LIMB2] and not [n for n in score if n in ("conv3x3_wino", "conv3x3_wino_gn")]
    assert not [r for r in log if r[1] == "score" and r[0] == "gemm_split" and r[2]]
    assert [n for n in clfl if n in LIMB3] and not [n for n in clfl if n in LIMB2]


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_sample_math_bf16x3_twice(tmp_path):
    """``sample --config c10_sota --math bf16x3``, 3 EM steps, 2 images, synthetic checkpoint, twice: identical uint8."""
    import json
    from psld_amd import cli, ops as o
    from tests.conftest import GOLDEN
    with open(os.path.join(GOLDEN, "net_meta.json")) as fh:
        meta = json.load(fh)["c10_sota"]
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    ck = str(tmp_path / "synth.ckpt")
    torch.save({"state_dict": {**{"score_fn." + k: v for k, v in sd.items()}, **{"ema_score_fn." + k: v for k, v in sd.items()}},
                "global_step": 0, "epoch": 0}, ck)
    outs = [str(tmp_path / "o1"), str(tmp_path / "o2")]
    old = o.math_mode()
    try:
        for out in outs:
            o.set_math_mode("bf16x6")
            cli.main(["sample", "--config", "c10_sota", "--math", "bf16x3", f"evaluation.chkpt_path={ck}", "evaluation.n_samples=2",
                      "evaluation.batch_size=2", "evaluation.n_discrete_steps=3", f"evaluation.save_path={out}",
                      "evaluation.save_mode=np", "evaluation.seed=0"])
            assert o.math_mode() == "bf16x3"
    finally:
        o.set_math_mode(old)
    files = sorted(os.listdir(os.path.join(outs[0], "images")))
    assert files
    for f in files:
        a, b = np.load(os.path.join(outs[0], "images", f)), np.load(os.path.join(outs[1], "images", f))
        assert a.dtype == np.uint8 and a.shape == (2, 32, 32, 3)
        np.testing.assert_array_equal(a, b)
