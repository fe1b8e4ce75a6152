"""The three measurements of profiles/r16/nll.md, one JSON line each:

  kernel    psld_nll_score_loss against psld_sqerr_loss_f32 at [128, 6, 32, 32] (loss + gradient; two launches per call):
            device events around ``--calls`` back-to-back calls, the two ops alternating over ``--rounds`` rounds.
  step      one C10-SOTA train step (SDEWrapper.training_step + EMA, synthetic data) with weighting 'fid' against weighting
            'nll' + importance sampling, on twin networks in the same process, alternating blocks of steps; wall clock
            between device synchronisations.
  stability std / mean of the step loss over ``--loss-steps`` evaluations of the criterion on FIXED weights (no optimiser
            step) under weighting 'nll', with the times drawn uniformly and through the importance density.

    python tools/nll_measure.py [--batch 128] [--config c10_sota]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import psld_amd  # noqa: E402
from psld_amd import config as C, ops  # noqa: E402
from psld_amd.optim import EMAWeightUpdate  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402


def kernel_times(dev, shape, calls, rounds):
    cfg = C.c10_sota()
    sde = get_module("sde", "psld")(cfg)
    b = shape[0]
    eps, pred = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
    t = torch.rand(b, device=dev, dtype=torch.float64) * (1 - 1e-5) + 1e-5
    tb = sde._coeff_table(t, 0, sde.mm_0)
    sw = torch.rand(b, device=dev, dtype=torch.float64) + 0.5
    run = {"sqerr": lambda: ops.sqerr_loss(eps, pred, True, want_grad=True),
           "nll": lambda: ops.nll_score_loss(eps, pred, t, tb, sw, sde._params, 0, True, want_grad=True)}
    us = {k: [] for k in run}
    for r in range(rounds + 1):                 # round 0 warms up
        for k, fn in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                us[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    return {"what": "kernel", "shape": list(shape), "calls": calls, "us_per_call": us, "median_us": med,
            "ratio_nll_over_sqerr": med["nll"] / med["sqerr"], "bytes_moved": 3 * eps.numel() * 4}


def _wrapper(cfg, net, sde):
    ema = copy.deepcopy(net)
    for p in ema.parameters():
        p.requires_grad = False
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    return get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema, criterion=crit)


def _cfgs(name, batch):
    fid = getattr(C, name)()
    fid.training.batch_size = batch
    nll = copy.deepcopy(fid)
    nll.training.loss.weighting = "nll"
    nll.training.loss.importance_sampling = True
    return fid, nll


def step_times(dev, name, batch, steps, rounds, warmup):
    cfgs = dict(zip(("fid", "nll_is"), _cfgs(name, batch)))
    size = cfgs["fid"].data.image_size
    torch.manual_seed(0)
    net0 = get_module("score_fn", "ncsnpp")(cfgs["fid"]).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(0)
    data = [torch.rand(batch, 3, size, size, device=dev, generator=g) * 2 - 1 for _ in range(4)]
    runs = {}
    for k, cfg in cfgs.items():
        net = copy.deepcopy(net0)
        runs[k] = (_wrapper(cfg, net, get_module("sde", "psld")(cfg)), EMAWeightUpdate(cfg.training.ema_decay), [0])
    del net0

    def block(k, n):
        wr, cb, count = runs[k]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = wr.training_step(data[count[0] % len(data)], count[0])
            cb.on_train_batch_end(None, wr)
            count[0] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, float(loss.detach())

    for k in runs:
        block(k, warmup)
    ms = {k: [] for k in runs}
    last = {}
    for _ in range(rounds):
        for k in runs:
            dt, last[k] = block(k, steps)
            ms[k].append(dt)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return {"what": "step", "config": name, "batch": batch, "steps_per_block": steps, "ms_per_step": ms, "median_ms": med,
            "ratio_nll_is_over_fid": med["nll_is"] / med["fid"], "last_loss": last}


def loss_stability(dev, name, batch, n):
    _, cfg = _cfgs(name, batch)
    size = cfg.data.image_size
    torch.manual_seed(0)
    net = get_module("score_fn", "ncsnpp")(cfg).to(dev).train()
    # the shipped initialisation ends in a zero convolution (init_scale = 0): give the output something to be wrong about
    with torch.no_grad():
        for p in net.parameters():
            if p.requires_grad and float(p.abs().max()) == 0:
                p.normal_(0, 0.02)
    net.weights_changed()
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.rand(batch, 3, size, size, device=dev, generator=g) * 2 - 1
    out = {"what": "stability", "config": name, "batch": batch, "evaluations": n}
    for on in (False, True):
        cfg.training.loss.importance_sampling = on
        wr = _wrapper(cfg, net, get_module("sde", "psld")(cfg))
        torch.manual_seed(5)
        vals = []
        for _ in range(n):
            _, t, weight = wr._draw_weighted_times(batch, dev)
            with torch.no_grad():
                vals.append(wr.criterion(x0, t, net, t_weight=weight))
        v = torch.stack(vals).cpu()
        out["importance_sampling" if on else "uniform"] = {"mean": v.mean().item(), "std": v.std().item(),
                                                           "std_over_mean": (v.std() / v.mean()).item()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c10_sota")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loss-steps", type=int, default=50)
    ap.add_argument("--only", default=None, choices=["kernel", "step", "stability"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nll_measure.py needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    psld_amd.import_modules_into_registry()
    ops.lib()
    if args.only in (None, "kernel"):
        print(json.dumps(kernel_times(dev, (args.batch, 6, 32, 32), args.calls, args.rounds)), flush=True)
    if args.only in (None, "stability"):
        print(json.dumps(loss_stability(dev, args.config, args.batch, args.loss_steps)), flush=True)
    if args.only in (None, "step"):
        print(json.dumps(step_times(dev, args.config, args.batch, args.steps, args.step_rounds, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
