"""Likelihood-weighted PSLD training, the host side: constructor rules, the tabulated time density
``PSLD.nll_time_table`` and a numpy twin of the device sampler (``psld_sample_times_f64``), which tests/test_nll_gpu.py
compares the kernel against.  No GPU here.

Unbiasedness gates: the importance estimator mean(weight f(t)) over the stratified grid u_i = (i + 1/2) / 2^16 is the midpoint
rule of a smooth integrand in u on each bin; against the analytic / quadrature references it measured <= 3.8e-6 (f = t^-1/2)
and <= 2.9e-6 (f = w) relative for the C10-SOTA constants, both tables, 64 and 256 bins; the gate is 1e-4."""
import math

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C


def sample_times_np(u, tab):
    """psld_sample_times_f64 in numpy float64, operation for operation."""
    u = np.asarray(u, dtype=np.float64)
    cum, le, mass = tab["cum"], tab["log_edges"], tab["mass"]
    k = np.clip(np.searchsorted(cum, u, side="right") - 1, 0, mass.size - 1)   # the largest bin with cum[k] <= u
    pk, dl = mass[k], le[k + 1] - le[k]
    r = (u - cum[k]) / pk
    t = np.clip(np.exp(le[k] + r * dl), tab["t_lo"], tab["t_hi"])
    return t, t * dl / (pk * tab["span"])


def weight_fn(orc, t, mm_0):
    """w(t) = g_x^2 (c11^2 + c12^2) + g_m^2 (c21^2 + c22^2) from the oracle's own cov / inv_coeff (float64, vectorised)."""
    tt = torch.from_numpy(np.asarray(t, dtype=np.float64))
    c11, c12, c21, c22 = orc.inv_coeff(orc.cov(0.0, mm_0, tt))
    beta = orc.beta_t(tt)
    w = beta * orc.gamma * (c11 ** 2 + c12 ** 2) + beta * orc.m * orc.nu * (c21 ** 2 + c22 ** 2)
    return w.numpy()


def _sde(cfg=None):
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    cfg = cfg or C.c10_sota()
    return get_module("sde", cfg.model.sde.name)(cfg), cfg


def _loss(cfg, sde):
    from psld_amd.registry import get_module
    return get_module("losses", cfg.training.loss.name)(cfg, sde)


def test_psld_score_loss_accepts_nll_weighting():
    sde, cfg = _sde()
    cfg.training.loss.weighting = "nll"
    crit = _loss(cfg, sde)
    assert crit.weighting == "nll" and crit.importance_sampling is False
    cfg.training.loss.importance_sampling = True
    assert _loss(cfg, sde).importance_sampling is True
    sde, cfg = _sde()                                   # the default stays what it was
    crit = _loss(cfg, sde)
    assert crit.weighting == "fid" and crit.importance_sampling is False


def test_nll_with_l1_raises():
    sde, cfg = _sde()
    cfg.training.loss.weighting, cfg.training.loss.l_type = "nll", "l1"
    with pytest.raises(ValueError, match="l2"):
        _loss(cfg, sde)


def test_importance_sampling_needs_nll_and_psld():
    sde, cfg = _sde()
    cfg.training.loss.importance_sampling = True        # weighting is still 'fid'
    with pytest.raises(ValueError, match="importance_sampling"):
        _loss(cfg, sde)
    from psld_amd.registry import get_module
    with pytest.raises(ValueError, match="importance_sampling"):
        get_module("pl_modules", "sde_wrapper")(cfg, sde, torch.nn.Linear(1, 1), criterion=None)
    for weighting in ("fid", "nll"):
        vp, vcfg = _sde(C.c10_vpsde())
        vcfg.training.loss.weighting = weighting
        vcfg.training.loss.importance_sampling = True
        with pytest.raises(ValueError, match="importance_sampling"):
            _loss(vcfg, vp)
        vcfg.training.loss.importance_sampling = False
        _loss(vcfg, vp)


def test_nll_with_fp16_record_math_raises():
    """The check reads the process's math settings on the host (no launch): constructor and forward both refuse."""
    from psld_amd import ops
    sde, cfg = _sde()
    cfg.training.loss.weighting = "nll"
    crit = _loss(cfg, sde)
    before = (ops.math_mode(), ops.record_math(), ops.record_f16())
    try:
        ops.set_math_mode("bf16x6")
        ops.set_record_math("bf16x3")
        _loss(cfg, sde)                                 # bf16x3 is allowed
        ops.set_record_f16(True)
        with pytest.raises(ValueError, match=r"nll.*f16"):
            _loss(cfg, sde)
        with pytest.raises(ValueError, match=r"nll.*f16"):
            crit(torch.zeros(1, 3, 8, 8), torch.full((1,), 0.5, dtype=torch.float64), None)
        cfg.training.loss.weighting = "fid"
        _loss(cfg, sde)                                 # fp16 training with the default weighting is untouched
    finally:
        ops.set_math_mode(before[0])
        ops.set_record_math(before[1])
        ops.set_record_f16(before[2])


TABLES = [(mode, bins) for mode in ("hsm", "dsm") for bins in (64, 256)]


def _table(mode, bins):
    sde, cfg = _sde()
    mm_0 = sde.mm_0 if mode == "hsm" else 0.0
    return sde, mm_0, sde.nll_time_table(cfg.training.train_eps, mm_0, bins=bins)


@pytest.mark.parametrize("mode,bins", TABLES)
def test_time_table_properties(mode, bins):
    sde, mm_0, tab = _table(mode, bins)
    assert tab["edges"].shape == tab["log_edges"].shape == tab["cum"].shape == (bins + 1,) and tab["mass"].shape == (bins,)
    assert all(tab[k].dtype == np.float64 for k in ("edges", "log_edges", "mass", "cum"))
    assert tab["edges"][0] == 1e-5 and tab["edges"][-1] == 1.0 and tab["t_lo"] == 1e-5 and tab["t_hi"] == 1.0
    assert tab["span"] == 1.0 - 1e-5
    assert np.all(np.diff(tab["edges"]) > 0)
    assert abs(tab["mass"].sum() - 1.0) < 1e-14 and np.all(tab["mass"] > 0)
    assert tab["cum"][0] == 0.0 and tab["cum"][-1] == 1.0 and np.all(np.diff(tab["cum"]) > 0)
    # the host weight is the oracle's
    orc = O.PSLDOracle.from_config(C.c10_sota())
    for t in (1e-5, 1e-3, 0.3, 1.0):
        assert abs(sde.nll_weight_host(t, mm_0) - weight_fn(orc, [t], mm_0)[0]) <= 1e-12 * weight_fn(orc, [t], mm_0)[0]


def test_time_table_follows_the_score_mode():
    """Only the rows of L^{-T} the score mode uses enter the weight (score_m lower: c22 alone)."""
    cfg = C.c10_sota()
    cfg.model.sde.nu, cfg.model.sde.gamma = 4.0, 0.0
    sde, _ = _sde(cfg)
    orc = O.PSLDOracle.from_config(cfg)
    tt = torch.tensor([0.01, 0.5], dtype=torch.float64)
    c22 = orc.inv_coeff(orc.cov(0.0, sde.mm_0, tt))[3]
    want = (orc.beta_t(tt) * orc.m * orc.nu * c22 ** 2).numpy()
    got = np.array([sde.nll_weight_host(float(t), sde.mm_0) for t in tt])
    assert np.allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("mode,bins", TABLES)
def test_importance_estimator_is_unbiased(mode, bins):
    sde, mm_0, tab = _table(mode, bins)
    orc = O.PSLDOracle.from_config(C.c10_sota())
    eps, T = tab["t_lo"], tab["t_hi"]
    u = (np.arange(2 ** 16) + 0.5) / 2 ** 16
    t, wt = sample_times_np(u, tab)
    assert t.min() >= eps and t.max() <= T
    # E_U[t^-1/2] in closed form
    want = 2 * (math.sqrt(T) - math.sqrt(eps)) / (T - eps)
    got = np.mean(wt * t ** -0.5)
    print(f"{mode} {bins}: t^-1/2 rel err {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-4 * want
    # E_U[w]: trapezoid of w(t) t in ln t on 2^20 points
    lg = np.linspace(math.log(eps), math.log(T), 2 ** 20)
    f = weight_fn(orc, np.exp(lg), mm_0) * np.exp(lg)
    want = float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(lg))) / (T - eps)
    got = np.mean(wt * weight_fn(orc, t, mm_0))
    print(f"{mode} {bins}: w rel err {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-4 * want
    # the point of it: weight * w is nearly constant, where w alone under uniform times is not
    ur = np.random.RandomState(0).random_sample(2 ** 16)
    tr, wr = sample_times_np(ur, tab)
    v = wr * weight_fn(orc, tr, mm_0)
    cv = v.std() / v.mean()
    wu = weight_fn(orc, eps + ur * (T - eps), mm_0)
    print(f"{mode} {bins}: CV of weight*w {cv:.3f}; of w under uniform times {wu.std() / wu.mean():.1f}")
    assert cv < 0.1


def test_sampler_twin_edge_cases():
    _, _, tab = _table("hsm", 64)
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0)], tab["cum"][1:-1]])
    t, wt = sample_times_np(u, tab)
    assert t[0] == tab["t_lo"] and abs(t[1] - tab["t_hi"]) <= 1e-12
    assert np.allclose(t[2:], tab["edges"][1:-1], rtol=1e-13, atol=0)          # u on a cum entry starts the next bin
    assert np.all(np.isfinite(wt)) and np.all(wt > 0)
