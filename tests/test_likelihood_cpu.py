"""Host side of the probability-flow likelihood (psld_amd/likelihood.py): no library launches.

* the cotangent coefficients - the transpose of the linear map eps -> -1/2 g^2 s(eps) - against torch.autograd through the
  oracle's ``get_score`` (all three PSLD score modes, and the VP-SDE), 1e-12 relative;
* the momentum entropy, the bits/dim conversion and the linear divergence on hand-computed values;
* the ``bpd`` command's parser."""
import math

import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from psld_amd import likelihood as L
from psld_amd.sde import PSLD
from psld_amd.vpsde import VPSDE

T_VALUES = (1e-3, 0.3, 0.999)


def _psld_cfg(mode):
    cfg = C.tiny()
    s = cfg.model.sde
    if mode == "score_m":
        s.gamma, s.nu, s.decomp_mode = 0.0, 4.0, "lower"
    elif mode == "score_x":
        s.gamma, s.nu, s.decomp_mode = 4.0, 0.0, "upper"
    return cfg


@pytest.mark.parametrize("mode", ["score_xm", "score_m", "score_x"])
@pytest.mark.parametrize("t", T_VALUES)
def test_psld_cotangent_coefficients_against_autograd(mode, t):
    cfg = _psld_cfg(mode)
    sde, orc = PSLD(cfg), O.PSLDOracle.from_config(cfg)
    assert sde.mode == orc.mode == mode
    g = torch.Generator().manual_seed(3)
    full = mode == "score_xm"
    eps = torch.randn(1, 6 if full else 3, 4, 4, generator=g, dtype=torch.float64, requires_grad=True)
    z = torch.randn(1, 6, 4, 4, generator=g, dtype=torch.float64)
    tt = torch.tensor([t], dtype=torch.float64)
    _, gdiff = orc.sde(torch.zeros(1, 6, 4, 4, dtype=torch.float64), tt)
    a_eps = -0.5 * gdiff ** 2 * orc.get_score(eps, 0.0, orc.mm_0, tt)       # the score part of the probability-flow drift
    (w_ref,) = torch.autograd.grad((a_eps * z).sum(), eps)
    axx, axm, amx, amm = L.psld_cotangent_coeffs(sde, t)
    zx, zm = z[:, :3], z[:, 3:]
    if mode == "score_m":
        assert (axx, axm, amx) == (0.0, 0.0, 0.0)
        w = amm * zm
    elif mode == "score_x":
        assert (axm, amx, amm) == (0.0, 0.0, 0.0)
        w = axx * zx
    else:
        w = torch.cat([axx * zx + axm * zm, amx * zx + amm * zm], dim=1)
    assert w.shape == w_ref.shape
    err = (w - w_ref).abs().max().item()
    assert err <= 1e-12 * w_ref.abs().max().item(), (err, w_ref.abs().max().item())


@pytest.mark.parametrize("t", T_VALUES)
def test_vp_cotangent_coefficient_against_autograd(t):
    cfg = C.tiny_vpsde()
    sde, orc = VPSDE(cfg), O.VPSDEOracle(cfg.model.sde.beta_min, cfg.model.sde.beta_max)
    g = torch.Generator().manual_seed(4)
    eps = torch.randn(1, 3, 4, 4, generator=g, dtype=torch.float64, requires_grad=True)
    z = torch.randn(1, 3, 4, 4, generator=g, dtype=torch.float64)
    tt = torch.tensor([t], dtype=torch.float64)
    _, gdiff = orc.sde(torch.zeros_like(z), tt)
    a_eps = -0.5 * gdiff ** 2 * orc.get_score(eps, tt)
    (w_ref,) = torch.autograd.grad((a_eps * z).sum(), eps)
    w = L.vp_cotangent_coeff(sde, t) * z
    assert (w - w_ref).abs().max().item() <= 1e-12 * w_ref.abs().max().item()


def test_linear_divergence_by_hand():
    cfg = C.tiny()
    sde = PSLD(cfg)
    beta = sde.beta_0 + 0.3 * (sde.beta_1 - sde.beta_0)
    assert L.linear_divergence(sde, 0.3, 192) == pytest.approx(-0.5 * beta * (sde.gamma + sde.nu) * 192, rel=1e-15)
    vp = VPSDE(C.tiny_vpsde())          # beta(t) = 0.1 + 19.9 t
    assert L.linear_divergence(vp, 0.5, 48) == pytest.approx(-0.5 * 10.05 * 48, rel=1e-14)


def test_entropy_and_bits_per_dim_by_hand():
    # H(N(0, s I_D)) = D/2 (log 2 pi + 1 + log s):  D = 4, s = 1/4 -> 2 (1.8378770664093453 + 1 - 1.3862943611198906)
    assert L.momentum_entropy(0.25, 4) == pytest.approx(2.0 * (1.8378770664093453 + 1.0 - 1.3862943611198906), rel=1e-14)
    assert L.momentum_entropy(1.0 / (2 * math.pi * math.e), 7) == pytest.approx(0.0, abs=1e-14)
    # logp = -D ln 2 nats is one bit per dimension; the [-1, 1] mapping adds log2(127.5) = log2(255) - 1 bits
    d = 3 * 32 * 32
    assert L.bits_per_dim(-d * math.log(2.0), d) == pytest.approx(1.0 + 7.994353436858858 - 1.0, rel=1e-14)
    assert L.bits_per_dim(0.0, d, levels=256.0) == 8.0
    lp = torch.tensor([-d * math.log(2.0), 0.0], dtype=torch.float64)
    out = L.bits_per_dim(lp, d)
    assert out.dtype == torch.float64 and out[0].item() == pytest.approx(7.994353436858858, rel=1e-14)
    assert L.LEVELS_NORM == 127.5


def test_pflikelihood_options():
    cfg = C.tiny()
    lik = L.PFLikelihood(cfg, PSLD(cfg), score_fn=None)
    assert (lik.rtol, lik.atol, lik.eps, lik.probe, lik.psld) == (1e-5, 1e-5, cfg.evaluation.eval_eps, "rademacher", True)
    vcfg = C.tiny_vpsde()
    lik = L.PFLikelihood(vcfg, VPSDE(vcfg), score_fn=None, rtol=1e-3, atol=1e-4, eps=1e-2, probe="gaussian")
    assert (lik.rtol, lik.atol, lik.eps, lik.probe, lik.psld) == (1e-3, 1e-4, 1e-2, "gaussian", False)
    with pytest.raises(ValueError):
        L.PFLikelihood(cfg, PSLD(cfg), score_fn=None, probe="uniform")
    with pytest.raises(RuntimeError, match="device tensors"):
        L.PFLikelihood(cfg, PSLD(cfg), score_fn=None).log_prob(torch.zeros(1, 6, 4, 4))


def test_bpd_cli_parser():
    from psld_amd import cli
    ap = cli.build_parser()
    a, rest = ap.parse_known_args(["bpd", "--config", "tiny", "--data", "x.npy", "--ckpt", "last.ckpt", "--n-probes", "3",
                                   "--n-momentum", "2", "--rtol", "1e-3", "--atol", "1e-4", "--math", "f32",
                                   "evaluation.batch_size=8"])
    assert (a.cmd, a.config, a.data, a.ckpt, a.n_probes, a.n_momentum, a.rtol, a.atol, a.math) == \
        ("bpd", "tiny", "x.npy", "last.ckpt", 3, 2, 1e-3, 1e-4, "f32")
    assert rest == ["evaluation.batch_size=8"]
    d, _ = ap.parse_known_args(["bpd"])
    assert (d.n_probes, d.n_momentum, d.rtol, d.atol, d.probe, d.dequantize, d.ckpt) == (1, 1, 1e-5, 1e-5, "rademacher", False, None)
    helps = [sp for act in ap._actions if hasattr(act, "choices") and isinstance(act.choices, dict)
             for name, sp in act.choices.items() if name == "bpd"]
    assert "RECORDING" in helps[0].format_help()        # --math: what it does not change is said in the help text
    s = cli.bpd_summary([3.0, 4.0, 5.0], [100, 200])
    assert s == {"bpd": 4.0, "bpd_stderr": pytest.approx(1.0 / math.sqrt(3.0)), "n_images": 3, "mean_nfe": 150.0}
