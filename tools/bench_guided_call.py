#!/usr/bin/env python
"""Cost of one guided network call (PosteriorScoreFn) per task, against the bare ``vjp_input`` it is built around.

One process, the calls alternating: every call warmed twice, then ``--rounds`` rounds in which each call in turn runs a window
of ``--window`` calls between two device events, the window ending in a device synchronise.  Per call: the median over the
rounds, [min, max], in ms; per task also the median of the window-by-window differences from the bare call of the same round.
Besides: the measure kernels alone on the same shapes.  Random (seeded) weights; times do not depend on them.

    python tools/bench_guided_call.py --batch 64 --tasks sr4,sr2,deconv,pool4 --out profiles/r21/guided_call.md
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psld_amd  # noqa: E402
from psld_amd import config as C, ops  # noqa: E402
from psld_amd.guidance import OPERATORS, PosteriorScoreFn, apply_operator  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

DEV = "cuda"


def window(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--config", default="c10_sota")
    ap.add_argument("--tasks", default="sr4,sr2,deconv,pool4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    psld_amd.import_modules_into_registry()
    ops.lib()
    cfg = getattr(C, args.config)()
    net = get_module("score_fn", "ncsnpp")(cfg)
    net.load_state_dict(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7))
    net = net.to(DEV).eval()
    sde = get_module("sde", cfg.model.sde.name)(cfg)
    size, b = cfg.data.image_size, args.batch
    g = torch.Generator().manual_seed(1)
    u32 = torch.cat([torch.rand(b, 3, size, size, generator=g) * 2 - 1,
                     torch.randn(b, 3, size, size, generator=g) * float(np.sqrt(sde.mm_0))], 1).to(DEV)
    x0 = (torch.rand(b, 3, size, size, generator=g) * 2 - 1).to(DEV)
    w = torch.randn(u32.shape, generator=g).to(DEV)
    tv = torch.full((b,), float(np.float32(0.3)), device=DEV)
    calls = {"bare vjp_input": lambda: net.vjp_input(u32, tv, w), "plain forward": lambda: net(u32, tv)}
    fronts = {}
    for task in args.tasks.split(","):
        psf = "gauss:1.5" if task == "deconv" else None
        fn = PosteriorScoreFn(net, sde, task, 0.05, psf=psf)
        fn.set_measurement(apply_operator(x0, task, psf=psf))
        fronts[task] = fn
        calls[f"guided {task}"] = lambda fn=fn: fn(u32, tv)
    times = {k: [] for k in calls}
    with torch.no_grad():
        for fn in calls.values():
            fn(), fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fn in calls.items():
                times[name].append(window(fn, args.window))
        # the measure kernels alone, on the shapes of the guided calls
        eps = net(u32, tv).contiguous()
        q = fronts[next(iter(fronts))].coeffs(float(tv[0]))
        alone = {}
        for task, fn in fronts.items():
            y, aux = fn._measurement_for(u32)
            op, k = OPERATORS[task]
            if task == "deconv":
                run = lambda y=y, aux=aux: ops.restore_deconv_measure(u32, eps, y, aux, q, q.sigma_y2, q.r2)
            elif task.startswith("sr"):
                run = lambda y=y, aux=aux, k=k: ops.restore_sr_measure(u32, eps, y, aux[0], aux[1], q, q.sigma_y2, q.r2, k)
            else:
                run = lambda y=y, aux=aux, op=op, k=k: ops.restore_measure(u32, eps, y, aux, op, k, q)
            run(), run()
            torch.cuda.synchronize()
            alone[task] = [window(run, 100) for _ in range(args.rounds)]
    med = lambda v: float(np.median(v))
    bare = times["bare vjp_input"]
    lines = [f"`python tools/bench_guided_call.py --batch {b} --window {args.window} --rounds {args.rounds} --config {args.config} "
             f"--tasks {args.tasks}` on {torch.cuda.get_device_name(0)}, math mode {ops.math_mode()}, record math {ops.record_math()}, "
             f"eval mode, state {tuple(u32.shape)}.", "",
             "| call | ms per call: median [min, max] over the windows | difference from the bare call of the same round: median [min, max] |",
             "|---|---|---|"]
    for name, v in times.items():
        d = [a - c for a, c in zip(v, bare)]
        lines.append(f"| {name} | {med(v):.3f} [{min(v):.3f}, {max(v):.3f}] | {med(d):+.3f} [{min(d):+.3f}, {max(d):+.3f}] |")
    lines += ["", f"Window-to-window spread of the bare call: {max(bare) - min(bare):.3f} ms.", "",
              f"| measure kernel alone, {b * 3} planes of {size} x {size} | us per launch: median [min, max] over windows of 100 |", "|---|---|"]
    for task, v in alone.items():
        lines.append(f"| {task} | {1e3 * med(v):.1f} [{1e3 * min(v):.1f}, {1e3 * max(v):.1f}] |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
