"""Generate the AFHQv2-128 inpainting-network (nf = 160) fixtures from the REAL reference (CPU path), build container only.

    python tools/gen_golden_afhq160.py    # writes tests/golden/net_afhq160.npz, tests/golden/afhq160_meta.json

* afhq160_meta.json: the configuration the reference inpaints AFHQv2-128 with - main/configs/dataset/afhqv2/afhqv2128_psld.yaml
  read as YAML, with the overrides of scripts_psld/sota/cond/afhqv2/sample_inpaint_psld.sh applied (data, score net, SDE and
  the sampling keys) - and the state-dict census (keys, shapes, parameter count) of the reference's NCSN++ built from it.
* net_afhq160.npz: eval forward of that network with tests/synth.py weights (seed 6100) at B = 1, the recipe of
  net_afhq128.npz.  Two runs write the same bytes.
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

from gen_golden_afhq import YAML, REF, _value  # noqa: E402
from ref_shim import import_reference  # noqa: E402
from psld_amd.config import Config  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SAMPLE_SH = os.path.join(REF, "scripts_psld", "sota", "cond", "afhqv2", "sample_inpaint_psld.sh")
SEED = 6100
EVAL_KEYS = ("stride_type", "n_discrete_steps", "batch_size", "sample_from")
torch.set_num_threads(8)


def reference_config():
    """The diffusion node of the reference's AFHQv2-128 inpainting run as a plain dict."""
    import yaml
    with open(YAML) as fh:
        diff = yaml.safe_load(fh)["diffusion"]
    # the sampling script's dataset.diffusion.* overrides that configure the network, the SDE and the sampler; paths,
    # checkpoints, devices, seeds and output naming are run bookkeeping
    keep = ("data.name", "data.norm", "data.hflip", "model.score_fn.", "model.sde.", "evaluation.sampler.name") + \
        tuple("evaluation." + k for k in EVAL_KEYS)
    with open(SAMPLE_SH) as fh:
        for key, val in re.findall(r"dataset\.diffusion\.([\w.]+)=(\S+)", fh.read()):
            if not key.startswith(keep):
                continue
            node = diff
            parts = key.split(".")
            for p in parts[:-1]:
                node = node[p]
            node[parts[-1]] = _value(val)
    diff["model"]["sde"]["numerical_eps"] = float(diff["model"]["sde"]["numerical_eps"])
    return diff


def main():
    util = import_reference()
    NCSNpp = util.get_module("score_fn", "ncsnpp")
    diff = reference_config()
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
    np.savez(os.path.join(OUT, "net_afhq160.npz"), x=x.numpy(), t=t.numpy(), y=y.numpy())
    ev = diff["evaluation"]
    meta = {
        "seed": SEED,
        "n_keys": len(ks),
        "n_params": int(sum(int(np.prod(s)) for _, s in ks)),
        "keys": [[k, list(s)] for k, s in ks],
        "diffusion": {
            "data": {k: diff["data"][k] for k in ("name", "image_size", "hflip", "num_channels", "norm")},
            "score_fn": dict(diff["model"]["score_fn"]),
            "sde": dict(diff["model"]["sde"]),
            "evaluation": {**{k: ev[k] for k in EVAL_KEYS}, "sampler": {"name": ev["sampler"]["name"]}},
        },
    }
    with open(os.path.join(OUT, "afhq160_meta.json"), "w") as fh:
        json.dump(meta, fh)
    print(f"net_afhq160.npz: |y| rms {y.pow(2).mean().sqrt().item():.4f}; {meta['n_params']} params, {meta['n_keys']} keys")


if __name__ == "__main__":
    main()
