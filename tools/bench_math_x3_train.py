"""Record math 'bf16x3' (two bf16 limbs in the passes that record a backward pass) against 'bf16x6', alternating
bf16x6, bf16x3, bf16x6, bf16x3, ... in ONE process:
  (a) one launch at B = 128: the Winograd-domain weight gradient 256->256 @32 / @16 / @8 and 512->256 @32 (two sources of
      256), the data gradient 256->256 @32 (HIP events, --iters launches after a warm-up launch, --repeats rounds);
  (b) --steps full HSM train steps (perturb + forward + loss + backward + clip + Adam + EMA) after --warmup steps, --repeats
      rounds: C10-SOTA at B = 128 and B = 16, CelebA-64 at B = 128 (--steps-rows to choose).
Seeded synthetic inputs; nothing is read from outside the tree.  The gate the project uses: the SLOWEST bf16x3 figure
against the FASTEST bf16x6 figure of a row.
    python tools/bench_math_x3_train.py [--iters 20] [--steps 10] [--warmup 5] [--repeats 3] [--steps-rows c10_sota:128,...]"""
import argparse
import copy
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psld_amd  # noqa: E402
from psld_amd import config as C, ops  # noqa: E402
from psld_amd.optim import EMAWeightUpdate  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402
from tools.bench_math_x3 import MODES, rel_l2, report, timeit  # noqa: E402

DEV = "cuda"


def launches(args):
    B = 128
    for c1, c2, cout, s in ((256, 0, 256, 32), (256, 0, 256, 16), (256, 0, 256, 8), (256, 256, 256, 32)):
        g = torch.Generator(device=DEV).manual_seed(c1 + c2 + s)
        x1 = torch.randn(B, s, s, c1, device=DEV, generator=g) + 0.25
        x2 = torch.randn(B, s, s, c2, device=DEV, generator=g) if c2 else None
        dy = torch.randn(B, s, s, cout, device=DEV, generator=g)
        d6, d3 = (torch.empty(cout, c1 + c2, 3, 3, device=DEV) for _ in range(2))
        fn = {"bf16x6": lambda: ops.conv3x3_wgrad_wino(dy, cout, x1, d6, x2=x2),
              "bf16x3": lambda: ops.conv3x3_wgrad_wino_x3(dy, cout, x1, d3, x2=x2)}
        t = {m: [] for m in MODES}
        for _ in range(args.repeats):
            for m in MODES:
                t[m].append(timeit(fn[m], args.iters))
        ns, _ = ops.conv3x3_wgrad_wino_plan(cout, c1 + c2, B, s, s)
        report(f"wgrad {c1 + c2}->{cout} @{s} B={B} ({ns} K splits; rel-L2 x3 vs x6 {rel_l2(d3, d6):.2e})", t)
    cin = cout = 256
    s = 32
    g = torch.Generator(device=DEV).manual_seed(11)
    dy = torch.randn(B, s, s, cout, device=DEV, generator=g)
    w = torch.randn(cout, cin, 3, 3, device=DEV, generator=g) * 0.05
    f6, f3 = ops.conv3x3_wino_frag(w, True), ops.conv3x3_wino_dgrad_frag_x3(w)
    y6, y3 = (torch.empty(B, s, s, cin, device=DEV) for _ in range(2))
    fn = {"bf16x6": lambda: ops.conv3x3_wino(dy, None, f6, cin, y6, None, allow_split=True),
          "bf16x3": lambda: ops.conv3x3_wino_x3(dy, None, f3, cin, y3, None, allow_split=True)}
    t = {m: [] for m in MODES}
    for _ in range(args.repeats):
        for m in MODES:
            t[m].append(timeit(fn[m], args.iters))
    report(f"dgrad {cout}->{cin} @{s} B={B} (rel-L2 x3 vs x6 {rel_l2(y3, y6):.2e})", t)


def train_steps(args):
    psld_amd.import_modules_into_registry()
    for row in args.steps_rows.split(","):
        name, batch = row.split(":")
        batch = int(batch)
        cfg = getattr(C, name)()
        cfg.training.batch_size = batch
        size = cfg.data.image_size
        g = torch.Generator(device=DEV).manual_seed(0)
        data = [torch.rand(batch, 3, size, size, device=DEV, generator=g) * 2 - 1 for _ in range(2)]
        t = {m: [] for m in MODES}
        final = {}
        for _ in range(args.repeats):
            for m in MODES:
                ops.set_record_math(m)
                # a network of its own per measurement, from the same seed: both modes time the same steps of the same run
                torch.manual_seed(cfg.training.seed)
                net = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
                ema = copy.deepcopy(net)
                for p in ema.parameters():
                    p.requires_grad = False
                sde = get_module("sde", "psld")(cfg)
                crit = get_module("losses", "psld_score_loss")(cfg, sde)
                wrapper = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema, criterion=crit)
                cb = EMAWeightUpdate(cfg.training.ema_decay)

                def run(n, first):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last = None
                    for i in range(n):
                        last = wrapper.training_step(data[(first + i) % len(data)], first + i)
                        cb.on_train_batch_end(None, wrapper)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, last
                run(args.warmup, 0)
                dt, last = run(args.steps, args.warmup)
                t[m].append(dt / args.steps)
                final[m] = float(last.item())
                ops.check_device_errors(torch.device(DEV, torch.cuda.current_device()))
                del wrapper, net, ema
                torch.cuda.empty_cache()
        report(f"train step {name} B={batch} ({args.steps} steps after {args.warmup}; final loss bf16x6 {final['bf16x6']:.5f}, "
               f"bf16x3 {final['bf16x3']:.5f})", t, 1e3, "ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps-rows", default="c10_sota:128,c10_sota:16,celeba64_sota:128")
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    ops.lib()
    old = ops.record_math()
    try:
        if not args.skip_launches:
            launches(args)
        if not args.skip_steps:
            train_steps(args)
    finally:
        ops.set_record_math(old)


if __name__ == "__main__":
    main()
