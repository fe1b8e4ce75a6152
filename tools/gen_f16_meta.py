"""Writes tests/golden/f16_meta.json: rel-L2 of the CPU oracle routed through the one-product fp16 arithmetic (tests/f16_ref.py),
and through the TF32-rounded yardstick, against the reference goldens - the bound of tests/test_math_f16_gpu.py's network
tests.  CPU only, run once: ``python tools/gen_f16_meta.py [name ...]``."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import psld_oracle as O          # noqa: E402
from psld_amd import config as C             # noqa: E402
from tests import f16_ref as F16             # noqa: E402
from tests.synth import synth_state_dict     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "f16_meta.json")


class _Patch:
    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def T(a):
    return torch.from_numpy(np.asarray(a))


def _meta(fname, key=None):
    with open(os.path.join(GOLDEN, fname)) as fh:
        m = json.load(fh)
    return m[key] if key else m


NETS = {"c10_sota": (lambda: _meta("net_meta.json", "c10_sota"), C.c10_sota, "net_c10_sota.npz"),
        "celeba64": (lambda: _meta("net_meta.json", "celeba64"), C.celeba64_sota, "net_celeba64.npz"),
        "afhqv2_128": (lambda: _meta("afhq_meta.json"), C.afhqv2_128, "net_afhq128.npz"),
        "afhqv2_128_inpaint": (lambda: _meta("afhq160_meta.json"), C.afhqv2_128_inpaint, "net_afhq160.npz")}


def run(name, rnd):
    base_f, base_t = O.F, O.torch
    F16.route_oracle(_Patch(), O, rnd)
    try:
        if name.startswith("em_"):
            stride = name[3:]
            g = np.load(os.path.join(GOLDEN, "em_c10_sota.npz"))
            cfg = C.c10_sota()
            sde = O.PSLDOracle.from_config(cfg)
            meta = _meta("net_meta.json", "c10_sota")
            sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
            ts, n = O.sampling_times(sde.T, cfg.evaluation.eval_eps, 4, True, stride)
            with torch.no_grad():
                x = O.em_sample(sde, lambda u, tt: O.ncsnpp_forward(sd, cfg, u, tt), T(g[f"batch_{stride}"]), ts, n, True,
                                cfg.evaluation.eval_eps, noise=list(T(g[f"noise_{stride}"])))
            return rel_l2(x, T(g[f"x_{stride}"]))
        meta_f, cfg_f, gname = NETS[name]
        meta, g = meta_f(), np.load(os.path.join(GOLDEN, gname))
        sd = synth_state_dict([(k, tuple(s)) for k, s in meta["keys"]], meta["seed"])
        with torch.no_grad():
            y = O.ncsnpp_forward(sd, cfg_f(), T(g["x"]), T(g["t"]))
        return rel_l2(y, T(g["y"]))
    finally:
        O.F, O.torch = base_f, base_t


def main(names):
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    for name in names:
        t0 = time.time()
        out[name] = {"f16": run(name, F16.round_f16), "tf32": run(name, F16.round_tf32)}
        print(name, out[name], f"{time.time() - t0:.0f} s", flush=True)
        with open(OUT, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:] or list(NETS) + ["em_uniform", "em_quadratic"])
