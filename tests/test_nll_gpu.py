"""Likelihood-weighted PSLD training on the device: the loss kernel against a float64 restatement with
autograd, the time-sampler kernel against its numpy twin, PSLDScoreLoss(nll) through the tiny network against the CPU
oracle's composed loss, and the training step (eager and captured) under importance sampling.

Gates: loss 2e-5 relative (the gate of the VP-SDE nll loss test), gradients 1e-4 rel-L2 (the parity gate); the sampler 1e-13
relative (device and numpy exp / log differ by an ulp or two on exponents of magnitude <= 12)."""
import copy

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from tests.synth import synth_state_dict
from tests.test_nll_cpu import sample_times_np
from tests.test_oracle_golden import _net_cfg, _net_meta

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIMES = (1e-5, 1e-3, 0.5, 1.0)          # train_eps ... T
# score mode -> SDE constants: 0 = score_xm, 1 = score_m with the lower factor, 2 = score_x with the upper factor
SDES = {0: dict(nu=4.01, gamma=0.01, decomp_mode="lower"), 1: dict(nu=4.0, gamma=0.0, decomp_mode="lower"),
        2: dict(nu=0.0, gamma=4.0, decomp_mode="upper")}


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _psld(score_mode):
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    cfg = C.tiny()
    for k, v in SDES[score_mode].items():
        cfg.model.sde[k] = v
    sde = get_module("sde", "psld")(cfg)
    assert sde._score_mode() == score_mode
    return sde, O.PSLDOracle.from_config(cfg)


def _usable_times(orc, mm_0):
    """The times at which the oracle's own coefficients are finite (all four of TIMES for the constants above, both tables -
    checked on the CPU; the filter stays for modes 1 / 2 as a guard)."""
    keep = []
    for t in TIMES:
        tt = torch.tensor([t], dtype=torch.float64)
        try:
            var = orc.cov(0.0, mm_0, tt)
            cs = orc.coeff(var) + orc.inv_coeff(var)
        except ValueError:
            continue
        if all(bool(torch.isfinite(c).all()) for c in cs):
            keep.append(t)
    return keep


def _ref_loss(orc, eps, eps_pred, t, mm_0, sw, score_mode, mean):
    """float64 restatement: the f32-cast coefficients of get_score (psld.py:253-258), everything else in float64."""
    bc = lambda v: v.view(-1, 1, 1, 1)
    c11, c12, c21, c22 = (bc(c.float().double()) for c in orc.inv_coeff(orc.cov(0.0, mm_0, t)))
    gx2, gm2 = bc(orc.beta_t(t) * orc.gamma), bc(orc.beta_t(t) * orc.m * orc.nu)
    ex, em = torch.chunk(eps.double(), 2, dim=1)
    if score_mode == 0:
        px, pm = torch.chunk(eps_pred, 2, dim=1)
        dx = (-c11 * px - c12 * pm) - (-c11 * ex - c12 * em)
        dm = (-c21 * px - c22 * pm) - (-c21 * ex - c22 * em)
        per = gx2 * dx ** 2 + gm2 * dm ** 2
    elif score_mode == 1:
        per = gm2 * (-c22 * eps_pred + c22 * em) ** 2
    else:
        per = gx2 * (-c11 * eps_pred + c11 * ex) ** 2
    per = per.sum(dim=(1, 2, 3))
    loss = (per * sw).sum() if sw is not None else per.sum()
    return loss / eps.numel() if mean else loss


@pytest.mark.parametrize("table", ["hsm", "dsm"])
@pytest.mark.parametrize("score_mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(3, 3, 8, 8), (2, 1, 5, 5), (5, 3, 32, 32)])
def test_nll_loss_kernel_matches_float64_restatement(shape, score_mode, table):
    from psld_amd import ops
    sde, orc = _psld(score_mode)
    mm_0 = sde.mm_0 if table == "hsm" else 0.0
    times = _usable_times(orc, mm_0) if score_mode else list(TIMES)
    assert len(times) >= 2
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(1000 * score_mode + b * h)
    t = torch.tensor([times[i % len(times)] for i in range(b)], dtype=torch.float64)
    eps = torch.randn(b, 2 * c, h, w, generator=gen)
    tgt = eps if score_mode == 0 else torch.chunk(eps, 2, dim=1)[1 if score_mode == 1 else 0]
    pred = (tgt + 0.5 * torch.randn(tgt.shape, generator=gen)).contiguous()
    sw_all = torch.rand(b, generator=gen, dtype=torch.float64) * 3 + 0.1
    t_d, eps_d, pred_d = t.to(DEV), eps.to(DEV), pred.to(DEV)
    tb = sde._coeff_table(t_d, 0, mm_0)
    for mean in (True, False):
        for sw in (None, sw_all):
            p64 = pred.double().requires_grad_()
            want = _ref_loss(orc, eps, p64, t, mm_0, sw, score_mode, mean)
            want.backward()
            sw_d = sw.to(DEV) if sw is not None else None
            loss, grad = ops.nll_score_loss(eps_d, pred_d, t_d, tb, sw_d, sde._params, score_mode, mean, want_grad=True)
            loss2, grad2 = ops.nll_score_loss(eps_d, pred_d, t_d, tb, sw_d, sde._params, score_mode, mean, want_grad=True)
            assert loss.dtype == torch.float64 and loss.shape == () and grad.dtype == torch.float32
            assert grad.shape == pred.shape
            le = abs(loss.item() - want.item()) / abs(want.item())
            ge = rel_l2(grad, p64.grad)
            print(f"{shape} mode {score_mode} {table} mean={mean} sw={sw is not None}: loss {loss.item():.9e} rel {le:.2e}, "
                  f"grad rel-L2 {ge:.2e}")
            assert le < 2e-5
            assert ge < 1e-4
            assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
            only_loss, none = ops.nll_score_loss(eps_d, pred_d, t_d, tb, sw_d, sde._params, score_mode, mean, want_grad=False)
            assert none is None and torch.equal(only_loss, loss)


@pytest.mark.parametrize("mode,bins", [("hsm", 256), ("dsm", 64)])
def test_time_sampler_kernel_matches_numpy_twin(mode, bins):
    from psld_amd import ops
    sde, _ = _psld(0)
    tab = sde.nll_time_table(1e-5, sde.mm_0 if mode == "hsm" else 0.0, bins=bins)
    rs = np.random.RandomState(5)
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0)], tab["cum"][1:-1], rs.random_sample(4096)])
    dev = {k: torch.from_numpy(tab[k]).to(DEV) for k in ("cum", "log_edges", "mass")}
    args = (torch.from_numpy(u).to(DEV), dev["cum"], dev["log_edges"], dev["mass"], tab["span"], tab["t_lo"], tab["t_hi"])
    t, wt = ops.sample_times(*args)
    t2, wt2 = ops.sample_times(*args)
    assert t.dtype == wt.dtype == torch.float64 and torch.equal(t, t2) and torch.equal(wt, wt2)
    t_np, w_np = sample_times_np(u, tab)
    t, wt = t.cpu().numpy(), wt.cpu().numpy()
    print(f"{mode} {bins}: t rel {np.max(np.abs(t - t_np) / t_np):.2e}, weight rel {np.max(np.abs(wt - w_np) / w_np):.2e}")
    assert np.allclose(t, t_np, rtol=1e-13, atol=0) and np.allclose(wt, w_np, rtol=1e-13, atol=0)
    assert t.min() >= tab["t_lo"] and t.max() <= tab["t_hi"] and t[0] == tab["t_lo"]


def _tiny_net(train=True):
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    meta, cfg = _net_meta()["tiny"], _net_cfg("tiny")
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
    net = get_module("score_fn", "ncsnpp")(cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).train(train), cfg, sd


@pytest.mark.parametrize("mode", ["hsm", "dsm"])
def test_nll_loss_through_the_network_matches_the_composed_reference(mode):
    """PSLDScoreLoss(nll) - loss and every parameter gradient - against losses.py:55-63 composed with the oracle's get_score
    and likelihood weighting around ncsnpp_forward on the CPU (mean over B*2C*H*W, per-sample weights)."""
    import unittest.mock as mock
    from psld_amd.registry import get_module
    net, cfg, sd = _tiny_net()
    cfg.training.loss.weighting, cfg.training.mode = "nll", mode
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    orc = O.PSLDOracle.from_config(cfg)
    s = cfg.data.image_size
    gen = torch.Generator().manual_seed(21)
    x0 = torch.rand(2, 3, s, s, generator=gen) * 2 - 1
    eps = torch.randn(2, 6, s, s, generator=gen)
    m_unit = torch.randn(2, 3, s, s, generator=gen)
    t = torch.tensor([2e-3, 0.6], dtype=torch.float64)
    tw = torch.tensor([0.7, 1.9], dtype=torch.float64)
    # the reference's composition
    sd = {k: v.requires_grad_(not k == "all_modules.0.W") for k, v in sd.items()}
    m_0, mm_0 = (torch.zeros_like(x0), orc.mm_0) if mode == "hsm" else (np.sqrt(orc.mm_0) * m_unit, 0.0)
    z_t = orc.perturb_data(x0, m_0, 0, mm_0, t, eps)[0].type(torch.float32)
    eps_pred = O.ncsnpp_forward(sd, cfg, z_t, t.type(torch.float32))
    g2 = torch.cat([O.bcast(orc.beta_t(t) * orc.gamma, x0).expand(-1, 3, s, s),
                    O.bcast(orc.beta_t(t) * orc.m * orc.nu, x0).expand(-1, 3, s, s)], dim=1)
    err = (orc.get_score(eps_pred, 0, mm_0, t) - orc.get_score(eps, 0, mm_0, t)) ** 2 * g2
    want = torch.mean(err * tw.view(-1, 1, 1, 1))
    assert want.dtype == torch.float64
    want.backward()
    # the product path
    m_dev = m_unit.to(DEV)
    with mock.patch("torch.randn_like", lambda x_, **kw: m_dev):
        loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV), t_weight=tw.to(DEV))
    assert loss.dtype == torch.float64
    le = abs(loss.item() - want.item()) / abs(want.item())
    loss.backward()
    # every parameter at the 1e-4 rel-L2 gate.  The key bias of an attention block (NIN_1.b) has an EXACTLY zero gradient (the
    # softmax does not see a constant added to every logit of a row): both sides then hold float32 rounding noise of terms
    # that cancel, and a relative error of noise against noise says nothing.  Such a parameter is held to one float32 ulp
    # (2^-23) of the whole gradient's norm instead - a floor that is ~1e-7 of the gate's scale for every other parameter.
    ref = {k: sd[k].grad for k, p in net.named_parameters() if p.requires_grad}
    total = torch.linalg.vector_norm(torch.stack([g.double().norm() for g in ref.values()])).item()
    floor = 2.0 ** -23 * total
    worst, bad = 0.0, []
    for k, p in net.named_parameters():
        if not p.requires_grad:
            assert p.grad is None
            continue
        diff = (p.grad.detach().double().cpu() - ref[k].double()).norm().item()
        rn = ref[k].double().norm().item()
        if rn > floor:
            worst = max(worst, diff / rn)
        if diff > 1e-4 * rn + floor:
            bad.append((k, diff, rn))
    print(f"{mode}: loss {loss.item():.9e} rel {le:.2e}; worst parameter-gradient rel-L2 {worst:.2e} "
          f"(total gradient norm {total:.3e}, floor {floor:.1e})")
    assert le < 2e-5
    assert not bad, bad
    assert worst < 1e-4


def test_nll_loss_publishes_its_divisor():
    """As _SqErr: the backward of the loss notes the divisor its gradient carries (B*2C*H*W for the mean in every score mode,
    1 for the sum) for the network's backward pass."""
    from psld_amd import losses, ops
    sde, _ = _psld(1)
    t = torch.tensor([0.3, 0.7], dtype=torch.float64, device=DEV)
    tb = sde._coeff_table(t, 0, sde.mm_0)
    eps = torch.randn(2, 6, 8, 8, device=DEV)
    for mean, want in ((True, 2 * 6 * 64), (False, 1)):
        pred = torch.randn(2, 3, 8, 8, device=DEV, requires_grad=True)
        ops.set_loss_divisor(None)
        losses._NllScoreErr.apply(pred, eps, t, tb, None, sde._params, 1, mean).backward()
        assert ops.loss_divisor() == want and pred.grad.dtype == torch.float32
    ops.set_loss_divisor(None)


def _wrapper(cfg, net, sde):
    from psld_amd.registry import get_module
    ema = copy.deepcopy(net)
    for p in ema.parameters():
        p.requires_grad = False
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    return get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema, criterion=crit), ema


def test_training_steps_with_importance_sampling():
    from psld_amd.registry import get_module
    net, cfg, _ = _tiny_net()
    cfg.training.loss.weighting = "nll"
    cfg.training.loss.importance_sampling = True
    sde = get_module("sde", "psld")(cfg)
    wr, _ = _wrapper(cfg, net, sde)
    before = net.flatten_parameters().clone()
    s = cfg.data.image_size
    torch.manual_seed(4)
    for i in range(3):
        x0 = torch.rand(4, 3, s, s, device=DEV) * 2 - 1
        loss = wr.training_step(x0, i)
        assert loss.dtype == torch.float64 and loss.shape == () and bool(torch.isfinite(loss))
        print(f"step {i}: loss {loss.item():.6e}")
    assert not torch.equal(before, net.flatten_parameters())
    assert bool(torch.isfinite(net.flatten_parameters()).all())


def test_importance_sampling_leaves_the_rng_draw_count_alone():
    """One step from the same seed with the sampler on and off: the next draw of the device generator is the same number."""
    from psld_amd.registry import get_module
    nxt = []
    for on in (False, True):
        net, cfg, _ = _tiny_net()
        cfg.training.loss.weighting = "nll"
        cfg.training.loss.importance_sampling = on
        sde = get_module("sde", "psld")(cfg)
        wr, _ = _wrapper(cfg, net, sde)
        s = cfg.data.image_size
        x0 = torch.rand(4, 3, s, s, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) * 2 - 1
        torch.manual_seed(17)
        wr.training_step(x0, 0)
        nxt.append(torch.rand(1, device=DEV).item())
    assert nxt[0] == nxt[1]


def test_captured_nll_step_is_bitwise_the_eager_step():
    """As test_graph_captured_training_step_is_bitwise_the_eager_step, under weighting 'nll' with importance sampling: the
    time mapping is launched inside the capture on the static t_ buffer, the float64 loss comes back through the poison
    path's zero.  6 steps: 2 eager warm-up steps, the capture, 3 replays."""
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.optim import EMAWeightUpdate
    from psld_amd.registry import get_module
    cfg = C.tiny(nf=128, ch_mult=(1, 1), attn_resolutions=(16,))
    cfg.training.optimizer.warmup = 4
    cfg.training.loss.weighting = "nll"
    cfg.training.loss.importance_sampling = True
    torch.manual_seed(3)
    net_a = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
    net_b = copy.deepcopy(net_a)
    sde = get_module("sde", "psld")(cfg)
    data = [torch.rand(4, 3, 16, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(i)) * 2 - 1 for i in range(6)]
    runs = []
    for net, graphs in ((net_a, False), (net_b, True)):
        wr, ema = _wrapper(cfg, net, sde)
        if graphs:
            wr.enable_graphs(True, warmup_steps=2)
        cb = EMAWeightUpdate(cfg.training.ema_decay)
        torch.manual_seed(11)
        losses = []
        for i in range(6):
            loss = wr.training_step(data[i], i)
            assert loss.dtype == torch.float64
            losses.append(loss.item())
            cb.on_train_batch_end(None, wr)
        opt = wr.optimizers()
        runs.append((losses, net.flatten_parameters().clone(), opt._m.clone(), opt._v.clone(), ema.flatten_parameters().clone(),
                     opt._step))
        if graphs:
            assert "graph" in next(iter(wr._graph_steps.values()))          # the captured path really ran
    (la, pa, ma, va, ea, sa), (lb, pb, mb, vb, eb, sb) = runs
    print("eager  losses", la)
    print("graph  losses", lb)
    assert all(np.isfinite(la)) and la == lb and sa == sb == 6
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb)


@pytest.mark.parametrize("graphs", [False, True])
def test_a_refused_nll_step_logs_nan(graphs):
    """As test_a_refused_step_leaves_the_parameters_untouched, for the float64 loss: with the device error word set the
    optimiser kernels leave parameters and moments alone and the step's loss comes back NaN (through the float32 zero the
    wrapper adds to it) - eager and captured; with the word cleared the next step trains again."""
    from psld_amd import ops
    from psld_amd.registry import get_module
    cfg = C.tiny(nf=128, ch_mult=(1, 1), attn_resolutions=(16,))
    cfg.training.loss.weighting = "nll"
    cfg.training.loss.importance_sampling = True
    torch.manual_seed(7)
    net = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
    wr, _ = _wrapper(cfg, net, get_module("sde", "psld")(cfg))
    if graphs:
        wr.enable_graphs(True, warmup_steps=2)
    data = [torch.rand(4, 3, 16, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(i)) * 2 - 1 for i in range(7)]
    step = lambda i: wr.training_step(data[i], i)
    for i in range(4):                       # two eager warm-up steps, the capture, one replay
        assert bool(torch.isfinite(step(i)))
    if graphs:
        assert "graph" in next(iter(wr._graph_steps.values()))
    opt = wr.optimizers()
    torch.cuda.synchronize()
    snap = [t.clone() for t in (net.flatten_parameters(), opt._m, opt._v)]
    word = ops.gn_team_sync(DEV)[:8].view(torch.int64)
    word.fill_(1)                            # what gn_bwd_team_kernel stores when a member gives up
    try:
        for i in (4, 5):
            loss = step(i)
            assert loss.dtype == torch.float64 and bool(torch.isnan(loss)), "a refused step must log NaN"
        torch.cuda.synchronize()
        for was, now in zip(snap, (net.flatten_parameters(), opt._m, opt._v)):
            assert torch.equal(was, now)
    finally:
        word.fill_(0)
    assert bool(torch.isfinite(step(6)))
    assert not torch.equal(snap[0], net.flatten_parameters())
