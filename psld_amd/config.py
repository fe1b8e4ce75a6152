"""Attribute-style config node accepted by every plug-in constructor.

The reference passes the Hydra/OmegaConf node ``config.dataset.diffusion`` to every
class and only ever uses attribute access on it (SURVEY.md Appendix C;
reference main/train_sde.py:25, main/eval/sample.py:31).  OmegaConf is not
available on the GPU box, so this module provides a tiny attr-dict with the same
access pattern plus the two north-star presets.  An OmegaConf ``DictConfig`` works
unchanged wherever a ``Config`` is accepted.

Key names and default values follow main/configs/dataset/cifar10/cifar10_psld.yaml:1-99;
``c10_sota`` applies the overrides of
scripts_psld/sota/uncond/cifar10/train_uncond_psld.sh:6-21 and ``celeba64_sota``
those of scripts_psld/sota/uncond/celeba64/train_uncond_psld.sh:7-20; ``afhqv2_128`` is
main/configs/dataset/afhqv2/afhqv2128_psld.yaml with the overrides of
scripts_psld/ablations/uncond/afhqv2/train_uncond_psld.sh, and ``afhqv2_128_inpaint`` adds those of
scripts_psld/sota/cond/afhqv2/sample_inpaint_psld.sh; ``c10_ablation`` and ``c10_vpsde`` are cifar10_psld.yaml /
cifar10_vpsde.yaml with the overrides of scripts_psld/ablations/uncond/cifar10/{train,sample}_uncond_{psld,vpsde}.sh (the
four-level networks of the paper's ablation tables and its VP-SDE baseline).
"""
from __future__ import annotations

import copy


class Config(dict):
    """dict with recursive attribute access (``cfg.model.score_fn.nf``)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        for k, v in list(self.items()):
            if isinstance(v, dict) and not isinstance(v, Config):
                self[k] = Config(v)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as e:
            raise AttributeError(name) from e

    def __setattr__(self, name, value):
        if isinstance(value, dict) and not isinstance(value, Config):
            value = Config(value)
        self[name] = value

    def __deepcopy__(self, memo):
        return Config(copy.deepcopy(dict(self), memo))

    def override(self, dotted: str, value):
        """``cfg.override("model.score_fn.nf", 64)`` — Hydra-style dotted override."""
        node = self
        parts = dotted.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = Config(value) if isinstance(value, dict) else value
        return self


def _yaml_defaults() -> dict:
    return {
        "data": {
            "root": "", "name": "cifar10", "image_size": 32, "hflip": True,
            "num_channels": 3, "norm": True, "return_target": False,
        },
        "model": {
            "pl_module": "sde_wrapper",
            "score_fn": {
                "name": "ncsnpp", "in_ch": 6, "out_ch": 6, "nonlinearity": "swish",
                "nf": 128, "ch_mult": [1, 2, 2, 2], "num_res_blocks": 4,
                "attn_resolutions": [16], "dropout": 0.1, "resamp_with_conv": True,
                "noise_cond": True, "fir": False, "fir_kernel": [1, 3, 3, 1],
                "skip_rescale": True, "resblock_type": "biggan", "progressive": "none",
                "progressive_input": "none", "progressive_combine": "sum",
                "embedding_type": "positional", "init_scale": 0.0, "fourier_scale": 16,
            },
            "sde": {
                "name": "psld", "beta_min": 8.0, "beta_max": 8.0, "nu": 4.01,
                "gamma": 0.01, "kappa": 0.04, "decomp_mode": "lower",
                "numerical_eps": 1e-9, "n_timesteps": 1000, "is_augmented": True,
            },
        },
        "training": {
            "seed": 0, "continuous": True, "mode": "hsm",
            "loss": {"name": "psld_score_loss", "l_type": "l2", "reduce_mean": True,
                     "weighting": "fid"},
            "optimizer": {"name": "Adam", "lr": 2e-4, "beta_1": 0.9, "beta_2": 0.999,
                          "weight_decay": 0, "eps": 1e-8, "warmup": 5000, "grad_clip": 1.0},
            "train_eps": 1e-5, "fp16": False, "use_ema": True, "ema_decay": 0.9999,
            "batch_size": 32, "epochs": 5000, "log_step": 1, "accelerator": "gpu",
            "devices": [0], "chkpt_interval": 1, "restore_path": "", "results_dir": "",
            "workers": 1, "chkpt_prefix": "",
        },
        "evaluation": {
            "sampler": {"name": "em_sde"}, "seed": 0, "chkpt_path": "", "save_path": "",
            "n_discrete_steps": 1000, "denoise": True, "eval_eps": 1e-3,
            "stride_type": "uniform", "use_pflow": False, "sample_from": "target",
            "accelerator": "gpu", "devices": [0], "n_samples": 50000, "workers": 2,
            "batch_size": 64, "save_mode": "image", "sample_prefix": "gpu",
            "path_prefix": "",
        },
    }


def yaml_default() -> Config:
    """The shipped YAML defaults (ch_mult=[1,2,2,2], nres=4, no fir, positional)."""
    return Config(_yaml_defaults())


def c10_sota() -> Config:
    """CIFAR-10 SOTA net: BASELINE.json configs[0..2,4] (SURVEY.md §8 'C10-SOTA')."""
    c = yaml_default()
    sf = c.model.score_fn
    sf.ch_mult = [2, 2, 2]
    sf.num_res_blocks = 8
    sf.dropout = 0.15
    sf.progressive_input = "residual"
    sf.fir = True
    sf.embedding_type = "fourier"
    c.training.batch_size = 16
    return c


def celeba64_sota() -> Config:
    """CelebA-64 net: BASELINE.json configs[3]."""
    c = yaml_default()
    c.data.name = "celeba"
    c.data.image_size = 64
    sf = c.model.score_fn
    sf.ch_mult = [1, 2, 2, 2]
    sf.num_res_blocks = 4
    sf.dropout = 0.1
    sf.progressive_input = "residual"
    sf.fir = True
    sf.embedding_type = "fourier"
    c.model.sde.nu = 4.005
    c.model.sde.gamma = 0.005
    c.training.batch_size = 16
    return c


def c10_ablation() -> Config:
    """The CIFAR-10 ablation network (four levels: 32, 16, 8 and 4x4 maps): cifar10_psld.yaml with the overrides of
    scripts_psld/ablations/uncond/cifar10/train_uncond_psld.sh (nf 128, [1,2,2,2], 2 res blocks, nu 4.02 / gamma 0.02, batch
    32, hsm); the evaluation node carries the values of sample_uncond_psld.sh (1000 uniform sscs_sde steps, batch 16)."""
    c = yaml_default()
    sf = c.model.score_fn
    sf.in_ch, sf.out_ch = 6, 6
    sf.nf = 128
    sf.ch_mult = [1, 2, 2, 2]
    sf.num_res_blocks = 2
    sf.attn_resolutions = [16]
    sf.dropout = 0.1
    sde = c.model.sde
    sde.beta_min, sde.beta_max = 8.0, 8.0
    sde.nu, sde.gamma, sde.kappa, sde.decomp_mode = 4.02, 0.02, 0.04, "lower"
    c.training.mode = "hsm"
    c.training.batch_size = 32
    ev = c.evaluation
    ev.sampler.name = "sscs_sde"
    ev.stride_type = "uniform"
    ev.n_discrete_steps = 1000
    ev.batch_size = 16
    ev.sample_from = "target"
    ev.n_samples = 10000
    ev.workers = 1
    ev.path_prefix = 1000
    return c


def c10_vpsde() -> Config:
    """The VP-SDE baseline on CIFAR-10: cifar10_vpsde.yaml with the overrides of
    scripts_psld/ablations/uncond/cifar10/train_uncond_vpsde.sh (3 channels in and out, nf 128, [1,2,2,2], 4 res blocks, beta
    0.1 / 20, score_loss, batch 32); the evaluation node carries sample_uncond_vpsde.sh (1000 quadratic em_sde steps, batch
    16).  NOTE: the reference's sampling scripts (sample_uncond_vpsde*.sh) rebuild the network with num_res_blocks = 2 -
    a checkpoint of theirs needs ``model.score_fn.num_res_blocks = 2`` set on this preset."""
    c = yaml_default()
    sf = c.model.score_fn
    sf.in_ch, sf.out_ch = 3, 3
    sf.nf = 128
    sf.ch_mult = [1, 2, 2, 2]
    sf.num_res_blocks = 4
    sf.attn_resolutions = [16]
    sf.dropout = 0.1
    c.model.sde = Config({"name": "vpsde", "beta_min": 0.1, "beta_max": 20, "n_timesteps": 1000, "is_augmented": False})
    c.training.loss.name = "score_loss"
    c.training.batch_size = 32
    ev = c.evaluation
    ev.sampler.name = "em_sde"
    ev.stride_type = "quadratic"
    ev.n_discrete_steps = 1000
    ev.batch_size = 16
    ev.sample_from = "target"
    ev.n_samples = 10000
    ev.workers = 1
    ev.path_prefix = 1000
    return c


def afhqv2_128() -> Config:
    """AFHQv2 at 128x128: afhqv2128_psld.yaml + scripts_psld/ablations/uncond/afhqv2/train_uncond_psld.sh (batch 8)."""
    c = yaml_default()
    c.data.name = "afhqv2"
    c.data.image_size = 128
    c.data.hflip = True
    c.data.norm = True
    sf = c.model.score_fn
    sf.nf = 128
    sf.ch_mult = [1, 2, 2, 2, 3]
    sf.num_res_blocks = 2
    sf.attn_resolutions = [16]
    sf.dropout = 0.2
    sf.fir = False
    sf.progressive_input = "none"
    sf.embedding_type = "positional"
    sde = c.model.sde
    sde.nu, sde.gamma, sde.kappa, sde.decomp_mode = 4.01, 0.01, 0.04, "lower"
    c.training.optimizer.lr = 1e-4
    c.training.optimizer.warmup = 5000
    c.training.batch_size = 8
    return c


def afhqv2_128_inpaint() -> Config:
    """The SOTA AFHQv2-128 inpainting network: ``afhqv2_128`` with the score-net, SDE and evaluation overrides of
    scripts_psld/sota/cond/afhqv2/sample_inpaint_psld.sh (nf = 160, gamma = 0, 250 quadratic ip_em_sde steps)."""
    c = afhqv2_128()
    sf = c.model.score_fn
    sf.in_ch, sf.out_ch = 6, 3
    sf.nf = 160
    sf.ch_mult = [1, 2, 2, 3, 3]
    sf.num_res_blocks = 2
    sf.attn_resolutions = [8, 16]
    sf.dropout = 0.2
    sde = c.model.sde
    sde.beta_min, sde.beta_max = 8.0, 8.0
    sde.nu, sde.gamma, sde.kappa, sde.decomp_mode = 4.0, 0.0, 0.04, "lower"
    ev = c.evaluation
    ev.sampler.name = "ip_em_sde"
    ev.stride_type = "quadratic"
    ev.n_discrete_steps = 250
    ev.batch_size = 16
    ev.sample_from = "target"
    return c


def tiny(image_size: int = 16, nf: int = 32, ch_mult=(1, 2), num_res_blocks: int = 1,
         attn_resolutions=(8,)) -> Config:
    """Reduced net with every block kind of C10-SOTA (used by parity tests/smoke)."""
    c = c10_sota()
    c.data.image_size = image_size
    sf = c.model.score_fn
    sf.nf = nf
    sf.ch_mult = list(ch_mult)
    sf.num_res_blocks = num_res_blocks
    sf.attn_resolutions = list(attn_resolutions)
    sf.dropout = 0.0
    return c


def tiny_vpsde() -> Config:
    """Reduced VP-SDE baseline net (keys of main/configs/dataset/cifar10/cifar10_vpsde.yaml:10-40)."""
    c = tiny()
    sf = c.model.score_fn
    sf.in_ch = sf.out_ch = 3
    sf.fir = False
    sf.progressive_input = "none"
    sf.embedding_type = "positional"
    c.model.sde = Config({"name": "vpsde", "beta_min": 0.1, "beta_max": 20.0, "n_timesteps": 1000,
                          "is_augmented": False})
    c.training.loss.name = "score_loss"
    return c


# ---- classifier guidance: the ``clf`` node of cifar10_psld.yaml:101-170 -------------------------
def _clf_yaml_defaults() -> dict:
    return {
        "data": {"root": "", "name": "cifar10", "image_size": 32, "hflip": True, "num_channels": 3, "norm": True,
                 "return_target": True},
        "model": {
            "pl_module": "tclf_wrapper",
            "clf_fn": {
                "name": "ncsnpp_clf", "in_ch": 6, "nonlinearity": "swish", "nf": 128, "ch_mult": [1, 2, 2, 2],
                "num_res_blocks": 2, "attn_resolutions": [16], "dropout": 0.1, "resamp_with_conv": True,
                "noise_cond": True, "fir": False, "fir_kernel": [1, 3, 3, 1], "skip_rescale": True,
                "resblock_type": "biggan", "progressive": "none", "progressive_input": "none",
                "progressive_combine": "sum", "embedding_type": "positional", "init_scale": 0.0,
                "fourier_scale": 16, "n_cls": 10,
            },
        },
        "training": {
            "seed": 0, "continuous": True,
            "loss": {"name": "tce_loss", "l_type": "l2", "reduce_mean": True},
            "optimizer": {"name": "Adam", "lr": 2e-4, "beta_1": 0.9, "beta_2": 0.999, "weight_decay": 0,
                          "eps": 1e-8, "warmup": 5000},
            "fp16": False, "batch_size": 32, "epochs": 500, "log_step": 1, "accelerator": "gpu", "devices": [0],
            "chkpt_interval": 1, "restore_path": "", "results_dir": "", "workers": 1, "chkpt_prefix": "",
        },
        "evaluation": {"seed": 0, "chkpt_path": "", "accelerator": "gpu", "devices": [0], "workers": 1,
                       "batch_size": 64, "clf_temp": 1.0, "label_to_sample": 0},
    }


def clf_default() -> Config:
    """The shipped ``clf`` YAML node (n_cls is ``???`` there; 10 = CIFAR-10)."""
    return Config(_clf_yaml_defaults())


def clf_c10() -> Config:
    """Classifier of scripts_psld/ablations/cond/cifar10/{train,sample}_tclf_psld.sh."""
    c = clf_default()
    cf = c.model.clf_fn
    cf.ch_mult = [1, 2, 3, 4]
    cf.num_res_blocks = 4
    cf.attn_resolutions = [16, 8]
    cf.n_cls = 10
    return c


def clf_afhqv2_128() -> Config:
    """The ``clf`` node of afhqv2128_psld.yaml (n_cls is ``???`` there; 3 = AFHQv2's cat / dog / wild)."""
    c = clf_default()
    c.data.name = "afhqv2"
    c.data.image_size = 128
    cf = c.model.clf_fn
    cf.ch_mult = [1, 2, 2, 2]
    cf.num_res_blocks = 2
    cf.attn_resolutions = [16]
    cf.dropout = 0.1
    cf.n_cls = 3
    c.training.optimizer.lr = 2e-4
    return c


def tiny_clf(image_size: int = 16, nf: int = 32, ch_mult=(1, 2), num_res_blocks: int = 1,
             attn_resolutions=(8,), n_cls: int = 10) -> Config:
    """Reduced classifier with every block kind of the shipped one (parity tests)."""
    c = clf_default()
    c.data.image_size = image_size
    cf = c.model.clf_fn
    cf.nf, cf.ch_mult, cf.num_res_blocks = nf, list(ch_mult), num_res_blocks
    cf.attn_resolutions, cf.n_cls, cf.dropout = list(attn_resolutions), n_cls, 0.0
    return c


def with_clf(diffusion: Config, clf: Config) -> Config:
    """Root node of the classifier-guidance apps (``config.dataset`` in main/train_clf.py:27 and
    main/eval/class_cond_sample.py:33): ``.diffusion`` and ``.clf`` side by side."""
    return Config({"diffusion": diffusion, "clf": clf})
