"""Class-conditional NCSN++ and classifier-free guidance on the GPU: the three kernels (label embedding add, its table
gradient, the guidance combine) against torch / fp64, the network against the CPU oracle with the label folded into the second
time-MLP bias, gradients, label dropout and its place in the RNG stream, training steps, CFGScoreFn under the samplers, graph
replay with changing labels, and the two commands.

Bounds.  u = 2^-24 (fp32 unit round-off).
  * label_embed_add: one fp32 add per element -> torch.equal with temb + table[lab].
  * label_embed_grad: a row's n_r terms are added one after the other, n_r - 1 roundings -> |err| <= n_r * u * sum|terms|.  The
    accumulate form adds the finished sum to the previous value, one more rounding, so the previous value counts as one more
    term: |err| <= n_r * u * (|prev| + sum|terms|), and a row without samples is its previous value bit for bit.
  * cfg_combine: out = fma(s, fl(c - u), u), two roundings -> |err| <= 4 * u * (|u| + |s| |c - u|).
  * network outputs and gradients against the oracle: the project's 1e-4 rel-L2 gate."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from tests import guard as G
from tests.synth import synth_state_dict
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
L2_BIAS = "all_modules.2.bias"          # the second Linear of the time MLP in the (Fourier-embedding) tiny networks
SHAPES = [(1, 16, 1), (3, 128, 10), (130, 512, 1000), (5, 20, 3)]


@pytest.fixture(scope="module")
def ops():
    from psld_amd import ops as o
    o.lib()
    return o


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _label_cases(b, k, seed):
    """(name, labels int64 [b] in [0, k], drop uint8 [b] or None): mixed labels with and without a dropout mask, every sample
    dropped, every sample on one row."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, k + 1, (b,), generator=g)
    drop = (torch.rand(b, generator=g) < 0.4).to(torch.uint8)
    if b > 1:
        drop[0], drop[-1] = 1, 0
    return [("labels", lab, None), ("drop", lab, drop), ("all dropped", lab, torch.ones(b, dtype=torch.uint8)),
            ("one row", torch.full((b,), k // 2, dtype=torch.int64), None)]


def _rows(lab, drop, k):
    return lab if drop is None else torch.where(drop.bool(), torch.full_like(lab, k), lab)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,d,k", SHAPES)
def test_label_embed_add(ops, b, d, k):
    temb, table = _rand(b, d, seed=1), _rand(k + 1, d, seed=2)
    for name, lab, drop in _label_cases(b, k, 3):
        ref = temb + table[_rows(lab, drop, k)]
        t = temb.to(DEV)
        out = ops.label_embed_add(t, table.to(DEV), lab.to(DEV), None if drop is None else drop.to(DEV))
        assert out is t and torch.equal(t.cpu(), ref), (name, (t.cpu() - ref).abs().max().item())
    # buffers that start 4 bytes past a 16-byte boundary take the one-float-per-thread form
    name, lab, drop = _label_cases(b, k, 3)[1]
    tb = torch.zeros(b * d + 1, device=DEV)[1:].view(b, d).copy_(temb)
    tab = torch.zeros((k + 1) * d + 1, device=DEV)[1:].view(k + 1, d).copy_(table)
    assert tb.data_ptr() % 16 == 4
    ops.label_embed_add(tb, tab, lab.to(DEV), drop.to(DEV))
    assert torch.equal(tb.cpu(), temb + table[_rows(lab, drop, k)])


@pytest.mark.parametrize("b,d,k", SHAPES)
def test_label_embed_grad(ops, b, d, k):
    dtemb = _rand(b, d, seed=4)
    cases = _label_cases(b, k, 5)
    dtable = torch.empty(k + 1, d, device=DEV)
    for i, (name, lab, drop) in enumerate(cases):
        # the buffer holds what the previous call left (the first time: a pattern) - every row is rewritten
        if i == 0:
            dtable.fill_(7.0)
        rows = _rows(lab, drop, k)
        args = (dtemb.to(DEV), lab.to(DEV), None if drop is None else drop.to(DEV))
        out = ops.label_embed_grad(*args, dtable)
        assert out is dtable
        got = dtable.cpu()
        again = ops.label_embed_grad(*args, torch.full_like(dtable, -3.0)).cpu()
        assert torch.equal(got, again), name                             # no atomics: bitwise reproducible
        count = torch.bincount(rows, minlength=k + 1)
        onehot = torch.zeros(k + 1, b, dtype=torch.float64)
        onehot[rows, torch.arange(b)] = 1.0
        ref = onehot @ dtemb.double()
        mag = onehot @ dtemb.double().abs()
        if bool((count == 0).any()):
            assert float(got[count == 0].abs().max()) == 0.0, name        # exact zeros over whatever the buffer held
        assert bool(((got.double() - ref).abs() <= count[:, None] * U * mag).all()), (name, (got.double() - ref).abs().max().item())
        # accumulate: previous + result; rows without samples keep their value bit for bit
        prev = _rand(k + 1, d, seed=6 + i)
        acc = prev.to(DEV)
        ops.label_embed_grad(*args, acc, accumulate=True)
        acc = acc.cpu()
        assert torch.equal(acc[count == 0], prev[count == 0]), name
        bound = count[:, None] * U * (prev.double().abs() + mag)
        assert bool(((acc.double() - (prev.double() + ref)).abs() <= bound).all()), name


@pytest.mark.parametrize("shape", [(3, 1, 1, 1), (1, 3, 5, 7), (2, 6, 16, 16), (5, 6, 33, 31), (4, 6, 32, 32)])
def test_cfg_combine(ops, shape):
    """Element counts 3, 105, 30690 (no multiple of 4: one float per thread) and 3072, 24576 (four per thread, several blocks)."""
    b = shape[0]
    eps2 = _rand(2 * b, *shape[1:], seed=8)
    c, u = eps2[:b].double(), eps2[b:].double()
    for s in (0.0, 1.0, 1.5, 7.5, -0.5):
        out = ops.cfg_combine(eps2.to(DEV), s)
        assert out.shape == shape and out.dtype == torch.float32
        ref = u + s * (c - u)
        err = (out.cpu().double() - ref).abs()
        bound = 4 * U * (u.abs() + abs(s) * (c - u).abs())
        assert bool((err <= bound).all()), (s, (err / bound.clamp_min(1e-300)).max().item())
    into = torch.empty(shape, device=DEV)
    assert ops.cfg_combine(eps2.to(DEV), 1.5, out=into) is into and torch.equal(into, ops.cfg_combine(eps2.to(DEV), 1.5))


@pytest.fixture(scope="module")
def pool():
    p = G.GuardPool(DEV, 64 << 20)
    yield p
    del p
    torch.cuda.empty_cache()


@pytest.mark.parametrize("b,d,k", [(3, 128, 10), (5, 20, 3), (130, 512, 1000)])
def test_guard_bands(ops, pool, monkeypatch, b, d, k):
    """No read or write outside the documented buffers (tests/guard.py): the three kernels on exactly-sized, banded buffers."""
    if pool.regions:
        pool.check()
        pool.release()
    guard = G.Guard(ops, pool).install(monkeypatch)
    _, lab, drop = _label_cases(b, k, 9)[1]
    lab, drop = lab.to(DEV), drop.to(DEV)
    temb, table = _rand(b, d, seed=10).to(DEV), _rand(k + 1, d, seed=11).to(DEV)
    for dr in (None, drop):
        G.run_guarded(guard, lambda temb, table, lab, drop: ops.label_embed_add(temb, table, lab, drop),
                      dict(temb=temb, table=table, lab=lab, drop=dr), ["temb"])
        for accumulate in (False, True):
            G.run_guarded(guard, lambda dtemb, lab, drop, dtable: ops.label_embed_grad(dtemb, lab, drop, dtable, accumulate),
                          dict(dtemb=temb, lab=lab, drop=dr, dtable=table), ["dtable"])
    for shape in ((2 * b, 3, 5, 7), (2 * b, 6, 4, 4)):
        G.run_guarded(guard, lambda eps2: ops.cfg_combine(eps2, 1.5), dict(eps2=_rand(*shape, seed=12).to(DEV)))
    assert guard.workspace_calls == 0
    pool.check()


# ---------------------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _build(cfg, sd):
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    net = get_module("score_fn", "ncsnpp")(cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


def _weights(nf, k, emb_scale=0.1):
    """(config of the conditional net, config of its unconditional twin, state dict of the twin, label table): the twin's
    weights are the synthetic ones of the other network tests, the table is random (its zero initialisation would hide it)."""
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    cfg0 = C.tiny(nf=nf)
    cfg = C.tiny(nf=nf)
    cfg.model.score_fn.label_classes = k
    keys = [(key, tuple(v.shape)) for key, v in get_module("score_fn", "ncsnpp")(cfg0).state_dict().items()]
    sd = synth_state_dict(keys, 7)
    return cfg, cfg0, sd, _rand(k + 1, 4 * nf, seed=21, scale=emb_scale)


def _net(nf, k=3):
    """(conditional network in eval mode, cfg, unconditional twin's cfg and CPU state dict, CPU label table), built once."""
    if (nf, k) not in _NETS:
        cfg, cfg0, sd, emb = _weights(nf, k)
        _NETS[nf, k] = _build(cfg, {"label_emb": emb, **sd}).eval(), cfg, cfg0, sd, emb
    return _NETS[nf, k]


def _shifted(sd, emb, r):
    """The unconditional twin that computes what label r does: the table row folded into the second time-MLP bias."""
    out = dict(sd)
    out[L2_BIAS] = sd[L2_BIAS] + emb[r]
    return out


def _inputs(b, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 6, 16, 16, generator=g), torch.rand(b, generator=g) * 0.9 + 0.05


@pytest.mark.parametrize("nf", [32, 128, 160])
def test_label_is_a_bias_shift(nf):
    """net(x, t, y) against the CPU oracle run on the shifted-bias state dict: a uniform label at B = 2, mixed labels (the
    "no label" row among them) sample by sample at B = 1; y=None is y = K everywhere, bit for bit."""
    net, cfg, cfg0, sd, emb = _net(nf)
    assert emb.shape == (4, 4 * nf) and sd[L2_BIAS].shape == (4 * nf,)
    x, t = _inputs(2, 31)
    with torch.no_grad():
        y = net(x.to(DEV), t.to(DEV), y=torch.full((2,), 1, device=DEV, dtype=torch.int64))
        ref = O.ncsnpp_forward(_shifted(sd, emb, 1), cfg0, x, t)
        e = rel_l2(y, ref)
        print(f"nf {nf}: uniform label 1 against the shifted-bias oracle: rel-L2 {e:.3e}")
        assert e < 1e-4
        assert rel_l2(y, O.ncsnpp_forward(sd, cfg0, x, t)) > 1e-4          # (the label does something the gate can see)
        x, t = _inputs(3, 32)
        labels = torch.tensor([2, 0, 3])
        y = net(x.to(DEV), t.to(DEV), y=labels.to(DEV))
        for i, r in enumerate(labels.tolist()):
            e = rel_l2(y[i:i + 1], O.ncsnpp_forward(_shifted(sd, emb, r), cfg0, x[i:i + 1], t[i:i + 1]))
            print(f"nf {nf}: sample {i} with label {r} against its B = 1 oracle: rel-L2 {e:.3e}")
            assert e < 1e-4
        none = net(x.to(DEV), t.to(DEV))
        assert torch.equal(none, net(x.to(DEV), t.to(DEV), y=torch.full((3,), 3, device=DEV, dtype=torch.int64)))


@pytest.mark.parametrize("nf", [32, 128])
def test_zero_table_is_the_unconditional_twin(nf):
    """label_emb all zero (its initialisation; an unconditional checkpoint loaded into a conditional network): the output is
    the unconditional network's bit for bit, whatever the labels - forward, and backward to every shared parameter and x."""
    cfg, cfg0, sd, emb = _weights(nf, 3)
    cond = _build(cfg, {"label_emb": torch.zeros_like(emb), **sd}).eval()
    twin = _build(cfg0, sd).eval()
    x, t = (v.to(DEV) for v in _inputs(3, 33))
    w = _rand(3, 6, 16, 16, seed=34).to(DEV)
    outs = []
    for net, kw in ((twin, {}), (cond, dict(y=torch.tensor([0, 3, 2], device=DEV))), (cond, {})):
        xr = x.clone().requires_grad_()
        out = net(xr, t, **kw)
        out.backward(w)
        outs.append((out.detach().clone(), xr.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
        for p in net.parameters():
            p.grad = None
    for out, dx, grads in outs[1:]:
        assert torch.equal(out, outs[0][0]) and torch.equal(dx, outs[0][1])
        assert set(grads) == set(outs[0][2]) | {"label_emb"}
        assert all(torch.equal(grads[k], v) for k, v in outs[0][2].items())
    with pytest.raises(ValueError, match="label_classes"):
        twin(x, t, y=torch.zeros(3, device=DEV, dtype=torch.int64))


def _oracle_grads(sd, cfg0, x, t, w):
    osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
    xr = x.clone().requires_grad_()
    O.ncsnpp_forward(osd, cfg0, xr, t).backward(w)
    return {k: v.grad for k, v in osd.items() if v.grad is not None}, xr.grad


@pytest.mark.parametrize("nf", [32, 128])
def test_gradients(nf):
    net, cfg, cfg0, sd, emb = _net(nf, 5)
    pd = dict(net.named_parameters())
    x, t = _inputs(4, 35)
    w = _rand(4, 6, 16, 16, seed=36)

    def backward(labels):
        for p in net.parameters():
            p.grad = None                       # the flat buffer keeps the last pass's values: the kernels overwrite them
        xr = x.to(DEV).requires_grad_()
        net(xr, t.to(DEV), y=labels.to(DEV)).backward(w.to(DEV))
        return xr.grad

    # distinct labels: every selected row of the table gradient is ONE sample's dtemb, so the rows are the terms of the bias
    # gradient's column sum; rows 1 and 3 have no sample
    backward(torch.tensor([2, 0, 5, 4]))
    ge = pd["label_emb"].grad.cpu().double()
    assert float(ge[[1, 3]].abs().max()) == 0.0 and all(float(ge[r].abs().max()) > 0 for r in (0, 2, 4, 5))
    gb = pd[L2_BIAS].grad.cpu().double()
    err = (ge.sum(0) - gb).abs()
    bound = 4 * U * ge.abs().sum(0)             # n = 4 samples
    print(f"nf {nf}: sum of label_emb.grad rows against the bias gradient: worst error / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    # a second backward with other labels: rows that are now unselected hold zeros, not the first pass's values
    backward(torch.tensor([1, 1, 3, 1]))
    ge2 = pd["label_emb"].grad.cpu()
    assert float(ge2[[0, 2, 4, 5]].abs().max()) == 0.0 and float(ge2[1].abs().max()) > 0 and float(ge2[3].abs().max()) > 0
    # the same through zero_grad()'s marker instead of dropped .grad tensors
    net.mark_grads_stale()
    xr = x.to(DEV).requires_grad_()
    net(xr, t.to(DEV), y=torch.tensor([0, 0, 0, 0], device=DEV)).backward(w.to(DEV))
    assert float(pd["label_emb"].grad[1:].abs().max()) == 0.0 and float(pd["label_emb"].grad[0].abs().max()) > 0
    # uniform label: every other gradient and dx against autograd through the shifted-bias oracle
    dx = backward(torch.full((4,), 2))
    og, odx = _oracle_grads(_shifted(sd, emb, 2), cfg0, x, t, w)
    total = torch.stack([v.double().norm() for v in og.values()]).norm().item()
    worst = ("dx", rel_l2(dx, odx))
    for k, ref in og.items():
        a = pd[k].grad
        if k.endswith("NIN_1.b"):       # analytically zero (softmax is shift-invariant): rounding noise, measured with the
            # floor the other network tests use for it
            e = ((a.double().cpu() - ref.double()).norm() / (ref.double().norm() + 1e-4 * total)).item()
        else:
            e = rel_l2(a, ref)
        worst = max(worst, (k, e), key=lambda v: v[1])
        assert e < 1e-4, (k, e)
    print(f"nf {nf}: uniform label against the shifted-bias oracle's autograd: worst rel-L2 {worst[1]:.3e} ({worst[0]})")
    assert worst[1] < 1e-4
    # the table's row 2 receives the bias gradient (every sample selects it)
    assert rel_l2(pd["label_emb"].grad[2], og[L2_BIAS]) < 1e-4


@pytest.mark.parametrize("nf", [32, 128])
def test_vjp_input_with_labels(nf):
    net, *_ = _net(nf)
    x, t = (v.to(DEV) for v in _inputs(3, 37))
    y = torch.tensor([1, 3, 0], device=DEV)
    w = _rand(3, 6, 16, 16, seed=38).to(DEV)
    fg = net.flat_grad()
    fg.copy_(torch.arange(fg.numel(), device=DEV, dtype=torch.float32) * 0.25 - 3.0)
    before = fg.clone()
    out, dx = net.vjp_input(x, t, w, y=y)
    assert torch.equal(fg, before), "vjp_input wrote into the flat gradient buffer"
    xr = x.clone().requires_grad_()
    full = net(xr, t, y=y)
    full.backward(w)
    assert torch.equal(out, full.detach()) and torch.equal(dx, xr.grad) and float(dx.abs().max()) > 0
    assert not torch.equal(fg, before)
    out0, dx0 = net.vjp_input(x, t, w)
    assert not torch.equal(out0, out) and not torch.equal(dx0, dx)          # y=None is another function
    for p in net.parameters():
        p.grad = None


# ---------------------------------------------------------------------------------------------------------------------
# loss and training step
# ---------------------------------------------------------------------------------------------------------------------
def _loss_setup(k, p=None):
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    cfg, cfg0, sd, emb = _weights(32, 3)
    if p is not None:
        cfg.training.label_dropout = p
    use = cfg if k else cfg0
    net = _build(use, {"label_emb": emb, **sd} if k else sd).train()
    sde = get_module("sde", "psld")(use)
    return net, get_module("losses", "psld_score_loss")(use, sde)


def test_loss_label_dropout_and_rng_order():
    g = torch.Generator().manual_seed(41)
    x0 = (torch.rand(4, 3, 16, 16, generator=g) * 2 - 1).to(DEV)
    eps = torch.randn(4, 6, 16, 16, generator=g).to(DEV)
    t = (torch.rand(4, generator=g, dtype=torch.float64) * 0.9 + 0.05).to(DEV)
    y = torch.tensor([0, 2, 1, 2], device=DEV)
    net, crit0 = _loss_setup(3, 0.0)
    assert crit0.label_dropout == 0.0
    by_hand = crit0(x0, t, lambda z, tt: net(z, tt, y=y), eps=eps)
    assert torch.equal(crit0(x0, t, net, eps=eps, y=y), by_hand)
    no_label = crit0(x0, t, net, eps=eps)
    assert not torch.equal(no_label, by_hand)
    _, crit1 = _loss_setup(3, 1.0)
    assert torch.equal(crit1(x0, t, net, eps=eps, y=y), no_label)
    # a drawn mask: the loss is the one with those samples on the "no label" row; the draw follows momentum and eps
    _, critp = _loss_setup(3, 0.5)
    torch.manual_seed(43)
    lp = critp(x0, t, net, y=y)
    torch.manual_seed(43)
    m_draw = torch.randn_like(x0)
    eps_d = torch.randn(4, 6, 16, 16, device=DEV)
    drop = torch.rand(4, device=DEV) < 0.5
    assert 0 < int(drop.sum()) < 4, "pick another seed: the mask should be mixed"
    assert torch.equal(lp, crit0(x0, t, net, eps=eps_d, m_draw=m_draw, y=torch.where(drop, torch.full_like(y, 3), y)))
    assert torch.equal(lp, crit0(x0, t, net, eps=eps_d, m_draw=m_draw, y=y, drop=drop))
    # the generator after a pass: labels with p > 0 cost exactly one rand(B); p = 0, y=None and a network without labels none
    def state_after(fn):
        torch.manual_seed(47)
        fn()
        return torch.cuda.get_rng_state()

    def draws(extra):
        torch.manual_seed(47)
        torch.randn_like(x0), torch.randn(4, 6, 16, 16, device=DEV)
        if extra:
            torch.rand(4, device=DEV)
        return torch.cuda.get_rng_state()

    net0, crit_u = _loss_setup(0)
    assert crit_u.label_dropout == 0.0
    plain = state_after(lambda: crit_u(x0, t, net0))
    assert torch.equal(plain, state_after(lambda: crit_u(x0, t, net0, y=None))) and torch.equal(plain, draws(False))
    assert torch.equal(plain, state_after(lambda: crit0(x0, t, net, y=y)))
    assert torch.equal(plain, state_after(lambda: critp(x0, t, net)))                 # y=None: nothing to drop
    assert torch.equal(state_after(lambda: critp(x0, t, net, y=y)), draws(True)) and not torch.equal(plain, draws(True))


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
def test_training_steps_touch_only_the_rows_they_saw(p_drop):
    """Three SDEWrapper.training_step((x0, y)) calls, K = 5, labels 0..2 only: finite losses; the rows seen move; without label
    dropout rows 3, 4 and the "no label" row stay bit for bit what they were (zero) in the parameters and in the EMA copy (with
    it the "no label" row moves too); and the same three steps with enable_graphs(True) - two eager warm-up steps, then the
    captured step, whose labels and dropout mask are refreshed static inputs - end at the same parameters, bit for bit, although
    the labels change per step."""
    import psld_amd
    from psld_amd.optim import EMAWeightUpdate
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    cfg, _, sd, emb = _weights(32, 5)
    cfg.training.label_dropout = p_drop
    cfg.training.optimizer.warmup = 0
    untouched = slice(3, None) if p_drop == 0 else slice(3, 5)
    ys = [torch.tensor(v, device=DEV) for v in ([0, 1, 0, 1], [1, 2, 2, 0], [0, 0, 1, 2])]
    data = [(torch.rand(4, 3, 16, 16, generator=torch.Generator().manual_seed(50 + i)) * 2 - 1).to(DEV) for i in range(3)]
    runs = []
    for graphs in (False, True):
        net = _build(cfg, {"label_emb": torch.zeros_like(emb), **sd}).train()
        ema = copy.deepcopy(net)
        for p in ema.parameters():
            p.requires_grad = False
        sde = get_module("sde", "psld")(cfg)
        wr = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema,
                                                     criterion=get_module("losses", "psld_score_loss")(cfg, sde))
        if graphs:
            wr.enable_graphs(True, warmup_steps=2)
        cb = EMAWeightUpdate(cfg.training.ema_decay)
        torch.manual_seed(53)
        losses = []
        for i in range(3):
            losses.append(wr.training_step((data[i], ys[i]), i).item())
            cb.on_train_batch_end(None, wr)
        assert all(np.isfinite(losses)), losses
        for m in (net, ema):
            e = m.label_emb.detach()
            if p_drop == 0:         # (under dropout a label's few occurrences may all have been dropped)
                assert all(float(e[r].abs().max()) > 0 for r in (0, 1, 2)), "a row that was seen did not move"
            assert float(e[untouched].abs().max()) == 0.0, "a row nobody selected changed"
        assert not torch.equal(net.state_dict()[L2_BIAS].cpu(), sd[L2_BIAS])
        opt = wr.optimizers()
        o = net._offsets[id(net.label_emb)]
        assert o == 0 and float(opt._m[:emb.numel()].view_as(emb)[untouched].abs().max()) == 0.0
        if graphs:
            ent = next(iter(wr._graph_steps.values()))
            assert "graph" in ent and ent["y"] is not None and (ent["drop"] is not None) == (p_drop > 0)   # the captured path ran
        runs.append((losses, net.flatten_parameters().clone(), ema.flatten_parameters().clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


# ---------------------------------------------------------------------------------------------------------------------
# classifier-free guidance
# ---------------------------------------------------------------------------------------------------------------------
def _two_pass(net, y, s):
    """The guidance in torch from two separate forwards."""
    def fn(x32, t32):
        c = net(x32, t32, y=y[:x32.shape[0]])
        u = net(x32, t32)
        return u + s * (c - u)
    return fn


@pytest.mark.parametrize("nf", [32, 128])
def test_cfg_score_fn(ops, monkeypatch, nf):
    from psld_amd.guidance import CFGScoreFn
    net, *_ = _net(nf)
    x, t = (v.to(DEV) for v in _inputs(3, 61))
    y = torch.tensor([2, 0, 1], device=DEV)
    calls = []
    combine = ops.cfg_combine
    monkeypatch.setattr(ops, "cfg_combine", lambda *a, **kw: calls.append(1) or combine(*a, **kw))
    with torch.no_grad():
        c, u = net(x, t, y=y), net(x, t)
        assert torch.equal(CFGScoreFn(net, y, 1.0)(x, t), c) and torch.equal(CFGScoreFn(net, y, 0.0)(x, t), u)
        assert torch.equal(CFGScoreFn(net, 1, 1.0)(x, t), net(x, t, y=torch.ones(3, device=DEV, dtype=torch.int64)))
        assert not calls
        for s in (2.5, -0.5):
            out = CFGScoreFn(net, y, s)(x, t)
            assert len(calls) == 1 and out.shape == c.shape
            calls.clear()
            ref = u.double() + s * (c.double() - u.double())
            mag = 4 * U * (u.double().abs() + abs(s) * (c.double() - u.double()).abs())
            e, allowed = rel_l2(out, ref), 1e-4 + (mag.norm() / ref.norm()).item()
            print(f"nf {nf}: CFG scale {s} from the doubled batch against two forwards: rel-L2 {e:.3e} (allowed {allowed:.3e})")
            assert e <= allowed
        # an int label, and a label tensor longer than the batch (the last, shorter batch of a run)
        long = torch.tensor([2, 0, 1, 1, 1], device=DEV)
        assert torch.equal(CFGScoreFn(net, long, 2.5)(x, t), CFGScoreFn(net, y, 2.5)(x, t))


@pytest.mark.parametrize("name", ["em_sde", "sscs_sde"])
def test_samplers_under_cfg(name):
    """Three steps (and the denoising step) of a sampler driven by CFGScoreFn against the same sampler driven by the two-pass
    torch callable, same noise: the existing 1e-5 rel-L2 parity bound of the EM sampler."""
    import psld_amd
    from psld_amd.guidance import CFGScoreFn
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    net, cfg, *_ = _net(32)
    cfg = copy.deepcopy(cfg)
    cfg.evaluation.n_discrete_steps = 3
    sde = get_module("sde", "psld")(cfg)
    g = torch.Generator().manual_seed(63)
    batch = torch.randn(2, 6, 16, 16, generator=g).to(DEV)
    noise = torch.randn(8, 2, 6, 16, 16, generator=g, dtype=torch.float64).to(DEV)
    ts = torch.linspace(0, 1.0 - 1e-3, 4, dtype=torch.float64, device=DEV)
    y = torch.tensor([1, 2], device=DEV)
    outs = []
    for fn in (CFGScoreFn(net, y, 1.5), _two_pass(net, y, 1.5), CFGScoreFn(net, y, 0.0)):
        sampler = get_module("samplers", name)(cfg, sde, fn)
        sampler.noise_fn = lambda i, x: noise[i]
        outs.append(sampler.sample(batch, ts, 3, denoise=True, eps=1e-3))
    e = rel_l2(outs[0], outs[1])
    print(f"{name}: 3 steps under CFGScoreFn against the two-pass callable: rel-L2 {e:.3e}")
    assert outs[0].dtype == torch.float64 and bool(torch.isfinite(outs[0]).all()) and e < 1e-5
    assert rel_l2(outs[2], outs[1]) > 1e-5                                  # (guidance changes the trajectory)


def test_graph_replay_follows_the_labels():
    """NCSNpp.enable_graphs: consecutive eval calls with different y (and y=None) return what the eager calls return."""
    cfg, _, sd, emb = _weights(32, 3)
    net = _build(cfg, {"label_emb": emb, **sd}).eval()
    x, t = (v.to(DEV) for v in _inputs(3, 65))
    ys = [torch.tensor(v, device=DEV) for v in ([0, 1, 2], [2, 2, 0], [3, 0, 1])] + [None]
    with torch.no_grad():
        eager = [net(x, t, y=y).clone() for y in ys]
        assert not torch.equal(eager[0], eager[1])
        net.enable_graphs(True)
        for y, ref in zip(ys + ys[:1], eager + eager[:1]):
            assert torch.equal(net(x, t, y=y), ref)
        assert len(net._graphs) == 1
        # the table is read where the optimiser writes it: a raw-pointer update shows in the next replay
        net.label_emb.data.mul_(2.0)
        out = net(x, t, y=ys[0])
        net.enable_graphs(False)
        assert torch.equal(out, net(x, t, y=ys[0])) and not torch.equal(out, eager[0])


# ---------------------------------------------------------------------------------------------------------------------
# commands
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_conditional_train_and_guided_sample(tmp_path):
    from psld_amd import cli
    res = str(tmp_path / "run")
    cond = ["--config", "tiny", "model.score_fn.label_classes=3"]
    cli.main(["train", *cond, "--labels", "synthetic", "--max-steps", "2", "--synthetic-size", "16", "--log-every", "1",
              "training.batch_size=4", "training.epochs=1", f"training.results_dir='{res}'", "training.chkpt_prefix=t"])
    ck = os.path.join(res, "checkpoints", "last.ckpt")
    state = torch.load(ck, map_location="cpu", weights_only=False)
    keys = list(state["state_dict"].keys())
    assert keys[0] == "score_fn.label_emb" and "ema_score_fn.label_emb" in keys and state["global_step"] == 2
    assert tuple(state["state_dict"]["score_fn.label_emb"].shape) == (4, 128)
    out = str(tmp_path / "s")
    cli.main(["sample", *cond, "--label", "1", "--cfg-scale", "2.0", f"evaluation.chkpt_path={ck}", "evaluation.n_samples=3",
              "evaluation.batch_size=2", "evaluation.n_discrete_steps=3", f"evaluation.save_path={out}", "evaluation.save_mode=np"])
    files = sorted(os.listdir(os.path.join(out, "images")))
    assert len(files) == 2
    assert [np.load(os.path.join(out, "images", f)).shape for f in files] == [(2, 16, 16, 3), (1, 16, 16, 3)]
    with pytest.raises(SystemExit, match="required"):
        cli.main(["train", *cond, "--max-steps", "1"])
    with pytest.raises(SystemExit, match="label_classes"):
        cli.main(["sample", "--config", "tiny", "--label", "1"])
    # a conditional checkpoint does not load into an unconditional network
    with pytest.raises(RuntimeError, match="label_emb"):
        cli.main(["sample", "--config", "tiny", f"evaluation.chkpt_path={ck}", "evaluation.n_samples=1"])


def test_unconditional_checkpoint_loads_into_a_conditional_network(tmp_path):
    """The one direction in which the key may be missing: the table keeps its zeros, so guided sampling from that checkpoint
    is the unconditional sampler's output, bit for bit."""
    from psld_amd import cli
    res = str(tmp_path / "run")
    cli.main(["train", "--config", "tiny", "--max-steps", "1", "--synthetic-size", "8", "training.batch_size=4",
              "training.epochs=1", f"training.results_dir='{res}'"])
    ck = os.path.join(res, "checkpoints", "last.ckpt")
    assert not any("label_emb" in k for k in torch.load(ck, map_location="cpu", weights_only=False)["state_dict"])
    common = [f"evaluation.chkpt_path={ck}", "evaluation.n_samples=2", "evaluation.batch_size=2", "evaluation.n_discrete_steps=3",
              "evaluation.save_mode=np"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    cli.main(["sample", "--config", "tiny", *common, f"evaluation.save_path={a}"])
    cli.main(["sample", "--config", "tiny", "model.score_fn.label_classes=3", "--label", "2", "--cfg-scale", "3.0", *common,
              f"evaluation.save_path={b}"])
    fa, fb = (sorted(os.listdir(os.path.join(d, "images"))) for d in (a, b))
    assert fa == fb and fa
    for f in fa:
        np.testing.assert_array_equal(np.load(os.path.join(a, "images", f)), np.load(os.path.join(b, "images", f)))
