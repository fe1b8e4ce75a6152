"""Generate the AFHQv2-128 fixtures from the REAL reference (CPU path), build container only.

    python tools/gen_golden_afhq.py       # writes tests/golden/net_afhq128.npz, tests/golden/afhq_meta.json

* afhq_meta.json: the configuration the reference trains AFHQv2-128 with - main/configs/dataset/afhqv2/afhqv2128_psld.yaml
  read as YAML, with the overrides of scripts_psld/ablations/uncond/afhqv2/train_uncond_psld.sh applied (the ``clf`` node
  as shipped, n_cls = 3) - and the state-dict census (keys, shapes, parameter count) of the reference's NCSN++ built from it.
* net_afhq128.npz: eval forward of that network with tests/synth.py weights (seed 6000), the recipe of net_c10_sota.npz, at
  B = 1 (two 128x128 images in and out would exceed the 1 MiB limit of a committed file).
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
YAML = os.path.join(REF_ROOT, "configs", "dataset", "afhqv2", "afhqv2128_psld.yaml")
TRAIN_SH = os.path.join(REF, "scripts_psld", "ablations", "uncond", "afhqv2", "train_uncond_psld.sh")
SEED = 6000
torch.set_num_threads(8)


def _value(text):
    import yaml
    v = yaml.safe_load(text.strip().strip("\\'\""))
    return v


def reference_config():
    """(diffusion node, clf node) of the reference's AFHQv2-128 run as plain dicts."""
    import yaml
    with open(YAML) as fh:
        root = yaml.safe_load(fh)
    diff, clf = root["diffusion"], root["clf"]
    # the train script's dataset.diffusion.* overrides; paths / devices / logging are run bookkeeping, not the model
    skip = ("data.root", "training.results_dir", "training.chkpt_prefix", "training.devices", "training.epochs",
            "training.chkpt_interval", "training.accelerator", "training.workers")
    with open(TRAIN_SH) as fh:
        for key, val in re.findall(r"dataset\.diffusion\.([\w.]+)=(\S+)", fh.read()):
            if key in skip:
                continue
            node = diff
            parts = key.split(".")
            for p in parts[:-1]:
                node = node[p]
            node[parts[-1]] = _value(val)
    for node in (diff["model"]["sde"],):
        node["numerical_eps"] = float(node["numerical_eps"])
    clf["model"]["clf_fn"]["n_cls"] = 3       # ``???`` in the YAML: AFHQv2 has three classes (cat, dog, wild)
    for opt in (diff["training"]["optimizer"], clf["training"]["optimizer"]):
        opt["lr"], opt["eps"] = float(opt["lr"]), float(opt["eps"])
    return diff, clf


def main():
    util = import_reference()
    NCSNpp = util.get_module("score_fn", "ncsnpp")
    diff, clf = reference_config()
    cfg = Config(json.loads(json.dumps(diff)))
    net = NCSNpp(cfg)
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(synth_state_dict(ks, SEED), strict=True)
    net.eval()
    g = torch.Generator().manual_seed(SEED + 7)
    x = torch.randn(1, cfg.model.score_fn.in_ch, 128, 128, generator=g)
    t = torch.rand(1, generator=g) * 0.98 + 0.01
    with torch.no_grad():
        y = net(x, t)
    np.savez(os.path.join(OUT, "net_afhq128.npz"), x=x.numpy(), t=t.numpy(), y=y.numpy())
    sel = lambda d, keys: {k: d[k] for k in keys}       # noqa: E731
    meta = {
        "seed": SEED,
        "n_keys": len(ks),
        "n_params": int(sum(int(np.prod(s)) for _, s in ks)),
        "keys": [[k, list(s)] for k, s in ks],
        "diffusion": {
            "data": sel(diff["data"], ("name", "image_size", "hflip", "num_channels", "norm")),
            "score_fn": {k: v for k, v in diff["model"]["score_fn"].items()},
            "sde": {k: v for k, v in diff["model"]["sde"].items()},
            "optimizer": {k: v for k, v in diff["training"]["optimizer"].items()},
            "training": sel(diff["training"], ("batch_size", "mode", "continuous", "use_ema", "ema_decay")),
            "loss": dict(diff["training"]["loss"]),
            "evaluation": sel(diff["evaluation"], ("batch_size", "n_discrete_steps", "eval_eps", "stride_type", "denoise")),
        },
        "clf": {
            "data": sel(clf["data"], ("name", "image_size", "hflip", "num_channels", "norm", "return_target")),
            "clf_fn": {k: v for k, v in clf["model"]["clf_fn"].items()},
            "optimizer": {k: v for k, v in clf["training"]["optimizer"].items()},
            "training": sel(clf["training"], ("batch_size", "epochs")),
        },
    }
    with open(os.path.join(OUT, "afhq_meta.json"), "w") as fh:
        json.dump(meta, fh)
    print(f"net_afhq128.npz: |y| rms {y.pow(2).mean().sqrt().item():.4f}; {meta['n_params']} params, {meta['n_keys']} keys")


if __name__ == "__main__":
    main()
