"""Generate the CIFAR-10 ablation / VP-SDE fixtures from the REAL reference (CPU path), build container only.

    python tools/gen_golden_c10abl.py     # writes tests/golden/c10abl_meta.json, net_c10_ablation.npz, net_c10_vpsde.npz

* c10abl_meta.json: the two configurations the reference trains the four-level CIFAR-10 networks with -
  main/configs/dataset/cifar10/cifar10_psld.yaml with the overrides of scripts_psld/ablations/uncond/cifar10/
  train_uncond_psld.sh ("c10_ablation") and cifar10_vpsde.yaml with those of train_uncond_vpsde.sh ("c10_vpsde"), each read
  as YAML; the ``evaluation`` node carries the evaluation overrides of the matching sample_uncond_*.sh - and the state-dict
  census (keys, shapes, parameter count) of the reference's NCSN++ built from each.
* net_c10_ablation.npz / net_c10_vpsde.npz: eval forward of those networks with tests/synth.py weights at B = 2, the recipe
  of net_c10_sota.npz.
"""
from __future__ import annotations

import json
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from ref_shim import REF_ROOT, import_reference  # noqa: E402
from psld_amd.config import Config  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
REF = os.path.dirname(REF_ROOT)
SCRIPTS = os.path.join(REF, "scripts_psld", "ablations", "uncond", "cifar10")
RUNS = {    # preset name -> (YAML, train script, sample script, seed of the synthetic weights)
    "c10_ablation": ("cifar10_psld.yaml", "train_uncond_psld.sh", "sample_uncond_psld.sh", 7000),
    "c10_vpsde": ("cifar10_vpsde.yaml", "train_uncond_vpsde.sh", "sample_uncond_vpsde.sh", 7100),
}
torch.set_num_threads(8)


def _value(text):
    import yaml
    return yaml.safe_load(text.strip().strip("\\'\""))


def _apply(diff, script, only=None):
    """The script's dataset.diffusion.* overrides (``only``: those below that node alone); paths / devices / logging are run
    bookkeeping, not the model."""
    skip = ("data.root", "training.results_dir", "training.chkpt_prefix", "training.devices", "training.epochs",
            "training.chkpt_interval", "training.accelerator", "training.workers", "evaluation.devices",
            "evaluation.save_path", "evaluation.chkpt_path")
    with open(os.path.join(SCRIPTS, script)) as fh:
        for key, val in re.findall(r"dataset\.diffusion\.([\w.]+)=(\S+)", fh.read()):
            if key in skip or (only is not None and not key.startswith(only + ".")):
                continue
            node = diff
            parts = key.split(".")
            for p in parts[:-1]:
                node = node[p]
            node[parts[-1]] = _value(val)


def reference_config(yaml_name, train_sh, sample_sh):
    """The diffusion node of one run as a plain dict."""
    import yaml
    with open(os.path.join(REF_ROOT, "configs", "dataset", "cifar10", yaml_name)) as fh:
        diff = yaml.safe_load(fh)["diffusion"]
    _apply(diff, train_sh)
    _apply(diff, sample_sh, only="evaluation")
    sde = diff["model"]["sde"]
    if "numerical_eps" in sde:
        sde["numerical_eps"] = float(sde["numerical_eps"])
    opt = diff["training"]["optimizer"]
    opt["lr"], opt["eps"] = float(opt["lr"]), float(opt["eps"])
    diff["evaluation"]["eval_eps"] = float(diff["evaluation"]["eval_eps"])
    diff["training"]["train_eps"] = float(diff["training"]["train_eps"])
    return diff


def main():
    util = import_reference()
    NCSNpp = util.get_module("score_fn", "ncsnpp")
    sel = lambda d, keys: {k: d[k] for k in keys if k in d}       # noqa: E731
    meta = {}
    for name, (yaml_name, train_sh, sample_sh, seed) in RUNS.items():
        diff = reference_config(yaml_name, train_sh, sample_sh)
        cfg = Config(json.loads(json.dumps(diff)))
        net = NCSNpp(cfg)
        ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict(synth_state_dict(ks, seed), strict=True)
        net.eval()
        size = cfg.data.image_size
        g = torch.Generator().manual_seed(seed + 7)
        x = torch.randn(2, cfg.model.score_fn.in_ch, size, size, generator=g)
        t = torch.rand(2, generator=g) * 0.98 + 0.01
        with torch.no_grad():
            y = net(x, t)
        np.savez(os.path.join(OUT, f"net_{name}.npz"), x=x.numpy(), t=t.numpy(), y=y.numpy())
        meta[name] = {
            "seed": seed,
            "n_keys": len(ks),
            "n_params": int(sum(int(np.prod(s)) for _, s in ks)),
            "keys": [[k, list(s)] for k, s in ks],
            "diffusion": {
                "data": sel(diff["data"], ("name", "image_size", "hflip", "num_channels", "norm")),
                "score_fn": dict(diff["model"]["score_fn"]),
                "sde": dict(diff["model"]["sde"]),
                "optimizer": dict(diff["training"]["optimizer"]),
                "training": sel(diff["training"], ("batch_size", "mode", "continuous", "use_ema", "ema_decay", "train_eps", "fp16")),
                "loss": dict(diff["training"]["loss"]),
                "evaluation": sel(diff["evaluation"], ("sampler", "batch_size", "n_discrete_steps", "eval_eps", "stride_type",
                                                       "denoise", "sample_from", "n_samples", "workers", "path_prefix",
                                                       "use_pflow", "seed", "sample_prefix")),
            },
        }
        print(f"net_{name}.npz: |y| rms {y.pow(2).mean().sqrt().item():.4f}; {meta[name]['n_params']} params, {len(ks)} keys")
    with open(os.path.join(OUT, "c10abl_meta.json"), "w") as fh:
        json.dump(meta, fh)


if __name__ == "__main__":
    main()
