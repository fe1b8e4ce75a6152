"""One right-hand-side evaluation of the likelihood ODE on the C10-SOTA network, two ways to the input gradient, alternating
(a), (b), (a), (b), ... in ONE process:
  (a) autograd   x.requires_grad_() through NCSNpp.forward and torch.autograd.grad: the full recorded backward - every weight,
                 bias and GroupNorm gradient computed and written into the flat gradient buffer next to dx;
  (b) vjp_input  NCSNpp.vjp_input: the same forward, the data-gradient launches of the backward alone.
Both include the cotangent and right-hand-side kernels (ops.pf_cotangent, ops.pf_div_rhs); dx of the two is compared bit
for bit.  Then one full PFLikelihood.log_prob at the same batch size: wall time and NFE.
HIP events, --iters evaluations after a warm-up evaluation, --repeats rounds.  Seeded synthetic weights; nothing is read
from outside the tree.  Reported: every round, the medians, and the SLOWEST (b) against the FASTEST (a).  --out writes
the report as markdown (profiles/r13/likelihood.md).
    python tools/bench_likelihood.py [--batch 64] [--iters 5] [--repeats 3] [--rtol 1e-5] [--atol 1e-5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import psld_amd  # noqa: E402
from psld_amd import config as C, ops  # noqa: E402
from psld_amd.likelihood import PFLikelihood  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

DEV = "cuda"


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-5)
    ap.add_argument("--atol", type=float, default=1e-5)
    ap.add_argument("--config", default="c10_sota")
    ap.add_argument("--no-log-prob", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    psld_amd.import_modules_into_registry()
    ops.lib()
    cfg = getattr(C, args.config)()
    net = get_module("score_fn", "ncsnpp")(cfg)
    net.load_state_dict(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7))
    net = net.to(DEV).eval()
    sde = get_module("sde", cfg.model.sde.name)(cfg)
    lik = PFLikelihood(cfg, sde, net, rtol=args.rtol, atol=args.atol)
    size, b = cfg.data.image_size, args.batch
    g = torch.Generator().manual_seed(1)
    u32 = torch.cat([torch.rand(b, 3, size, size, generator=g) * 2 - 1,
                     torch.randn(b, 3, size, size, generator=g) * float(np.sqrt(sde.mm_0))], 1).to(DEV)
    z = ops.rademacher(torch.empty_like(u32), seed=5)
    t = 0.3
    k, vp_std = lik._coeffs(float(np.float32(t)))
    tv = torch.full((b,), float(np.float32(t)), device=DEV)
    u64 = ops.f32_to_f64(u32)
    keep = {}

    def autograd_path():
        w = ops.pf_cotangent(z, k, vp_std)
        x = u32.detach().clone().requires_grad_()
        with torch.enable_grad():
            y = net(x, tv)
            (dx,) = torch.autograd.grad(y, x, grad_outputs=w)
        keep["a"] = dx
        return ops.pf_div_rhs(u64, y.detach(), dx, z, k, vp_std)

    def vjp_path():
        w = ops.pf_cotangent(z, k, vp_std)
        y, dx = net.vjp_input(u32, tv, w)
        keep["b"] = dx
        return ops.pf_div_rhs(u64, y, dx, z, k, vp_std)

    paths = {"a": autograd_path, "b": vjp_path}
    times = {"a": [], "b": []}
    for _ in range(args.repeats):
        for name in ("a", "b"):
            times[name].append(timeit(paths[name], args.iters))
    same = bool(torch.equal(keep["a"], keep["b"]))
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    lines = [f"# Likelihood right-hand side: input-gradient-only backward against the full backward",
             "",
             f"`python tools/bench_likelihood.py --batch {b} --iters {args.iters} --repeats {args.repeats} --rtol {args.rtol:g} --atol {args.atol:g}` on {torch.cuda.get_device_name(0)}, "
             f"config `{args.config}`, math mode {ops.math_mode()}, record math {ops.record_math()}, eval mode, B = {b}, "
             f"seeded synthetic weights.  One evaluation = cotangent kernel + network forward + backward to the input + "
             f"right-hand-side kernel; HIP events around {args.iters} evaluations per round, rounds alternate (a), (b).",
             "",
             "| path | rounds [ms] | median [ms] |",
             "|---|---|---|"]
    for n, label in (("a", "(a) autograd, full backward"), ("b", "(b) `vjp_input`, data gradients only")):
        lines.append(f"| {label} | {' '.join(f'{v * 1e3:.2f}' for v in times[n])} | {med[n] * 1e3:.2f} |")
    slow_b, fast_a = max(times["b"]), min(times["a"])
    lines += ["",
              f"Slowest (b) {slow_b * 1e3:.2f} ms against fastest (a) {fast_a * 1e3:.2f} ms: x{fast_a / slow_b:.3f} "
              f"({'(b) faster in every pairing' if slow_b < fast_a else '(b) NOT faster in every pairing'}); medians x{med['a'] / med['b']:.3f}.",
              f"`dx` of the two paths bit for bit equal: {same}.", ""]
    if not args.no_log_prob:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logp, nfe = lik.log_prob(u32, probes=z)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines += [f"One `PFLikelihood.log_prob` at B = {b}, rtol = atol = {args.rtol:g}, one Rademacher probe: {dt:.1f} s wall, NFE {nfe} "
                  f"({dt / nfe * 1e3:.1f} ms per evaluation, host and step controller included); mean log p {float(logp.mean()):.2f} nats "
                  "(synthetic weights: the figure says nothing about a trained model, and an untrained eps scaled by L_t^-T near "
                  "t = eps makes the ODE far costlier than a trained network's).", ""]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
