"""Writes tests/golden/f16_train_meta.json: the CPU oracle's parameter gradients under record f16 (tests/f16_train_ref.py:
one-product fp16 forward, shifted fp16 data gradient, two-limb weight gradient) against the fp32 oracle - global rel-L2 over
all parameter gradients, with the automatic gradient shift and with shift 0 - and the range census of the data-gradient
operands: what the rounding of dy * 2^shift meets at every convolution and einsum (largest magnitude, share of the non-zeros
below fp16's normal range 2^-14 and below half its smallest subnormal 2^-25, share clamped at 65504).  Synthetic weights
(tests/synth.py), B = 2.  CPU only, run once: ``python tools/gen_f16_train_meta.py [name ...]``."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import psld_oracle as O          # noqa: E402
from psld_amd import config as C             # noqa: E402
from tests import f16_train_ref as FT        # noqa: E402
from tests import x3_train_ref as XT         # noqa: E402
from tests.synth import synth_inputs, synth_state_dict     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "f16_train_meta.json")
NETS = {"tiny128": (lambda: C.tiny(nf=128, ch_mult=(1, 1)), 16), "c10_sota": (C.c10_sota, 32)}
SEED, INPUT_SEED, BATCH = 7, 3, 2


class _Patch:
    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def _keys(cfg):
    import psld_amd
    from psld_amd.registry import get_module
    psld_amd.import_modules_into_registry()
    net = get_module("score_fn", "ncsnpp")(cfg)
    return [(k, tuple(v.shape)) for k, v in net.state_dict().items()]


def grads(cfg, sd, inputs, route=None):
    """(loss, {name: gradient}, elements of the prediction) of the oracle's score loss; ``route(patch, oracle)`` routes its
    contractions first."""
    x0, eps, t = inputs
    base_f, base_t = O.F, O.torch
    if route is not None:
        route(_Patch(), O)
    try:
        osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
        numel = []

        def score_fn(z, tt):
            y = O.ncsnpp_forward(osd, cfg, z, tt)
            numel.append(y.numel())
            return y
        loss = O.psld_score_loss(O.PSLDOracle.from_config(cfg), x0, t, score_fn, eps)
        loss.backward()
        return loss.item(), {k: v.grad for k, v in osd.items() if v.grad is not None}, numel[0]
    finally:
        O.F, O.torch = base_f, base_t


def global_rel_l2(g, ref):
    num = torch.stack([(g[k].double() - ref[k].double()).norm() for k in ref]).norm().item()
    return num / torch.stack([ref[k].double().norm() for k in ref]).norm().item()


def summarise(rows):
    nz = sum(r["nonzero"] for r in rows)
    return {"sites": len(rows), "max_abs": max(r["max"] for r in rows),
            "worst_site_share_below_2m14": max(r["below_2m14"] / max(r["nonzero"], 1) for r in rows),
            "share_below_2m14": sum(r["below_2m14"] for r in rows) / nz,
            "share_below_2m25": sum(r["below_2m25"] for r in rows) / nz,
            "share_clamped": sum(r["clamped"] for r in rows) / nz,
            "smallest_site_median": min(r["median"] for r in rows)}


def run(name):
    cfg_f, size = NETS[name]
    cfg = cfg_f()
    sd = synth_state_dict(_keys(cfg), SEED)
    inputs = synth_inputs(BATCH, 3, size, seed=INPUT_SEED)
    assert cfg.training.loss.reduce_mean
    l32, g32, divisor = grads(cfg, sd, inputs)      # the divisor the loss applies: the prediction's element count (reduce_mean)
    auto = FT.shift_for(divisor)
    out = {"batch": BATCH, "divisor": divisor, "shift_auto": auto, "loss_f32": l32}
    for tag, shift in (("auto", auto), ("shift0", 0)):
        census = []
        loss, g, _ = grads(cfg, sd, inputs, lambda p, o: FT.route_oracle_autograd(p, o, shift, census))
        assert g.keys() == g32.keys()
        out[tag] = {"shift": shift, "loss": loss, "grads_rel_l2": global_rel_l2(g, g32), "census": summarise(census)}
    _, g2, _ = grads(cfg, sd, inputs, XT.route_oracle_autograd)
    out["two_limb_grads_rel_l2"] = global_rel_l2(g2, g32)
    return out


def main(names):
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    for name in names:
        t0 = time.time()
        out[name] = run(name)
        print(name, json.dumps(out[name], indent=1), f"{time.time() - t0:.0f} s", flush=True)
        with open(OUT, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:] or list(NETS))
