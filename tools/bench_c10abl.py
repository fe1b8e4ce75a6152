"""Timing of the four-level CIFAR-10 networks (maps 32, 16, 8 and 4x4) on the tree whose root is argv[1]
(profiles/r14/c10_ablation.md).

    python tools/bench_c10abl.py ROOT nets       # per network (ablation PSLD nres = 2, VP-SDE nres = 4) and batch (32, 128): ms of
                                                 # one train step (forward + loss + backward), of one EM sampling step (the em_sde
                                                 # sampler's predictor update: noise draw, network call, fused SDE update) and of
                                                 # the bare eval forward inside it
    python tools/bench_c10abl.py ROOT nets wino4 # the same with the 4x4 level on the Winograd kernels from batch 8 up
                                                 # (ops.set_winograd_4x4(1), trees that have it) - an A/B inside one tree
    python tools/bench_c10abl.py ROOT launches 32  # one batch only (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...)
    python tools/bench_c10abl.py ROOT launches   # the bare 3x3 launches of the 4x4 level, 256 -> 256 and 256 + 256 -> 256, at
                                                 # batches 8 .. 128: forward, data gradient, weight gradient - on the fp32 tile
                                                 # engine and, where the tree's kernels take 4x4 maps, in Winograd form

``launches`` also reports ``floor``: the same timing loop around a four-element ``ops.axpby`` - the interval at which this
host issues launches through the Python wrappers.  A figure near the floor is the host's issue rate, not kernel time.

ROOT may be another checkout of the project (built in place) so that two trees are timed on one box.  The configurations are
built from ``yaml_default()`` plus overrides, not from the ``c10_ablation`` / ``c10_vpsde`` presets, so the file runs unchanged
on trees that do not have them.  HIP events around ``iters`` back-to-back calls after a warm-up.
"""
import json
import os
import sys

root = sys.argv[1]
sys.path.insert(0, os.path.abspath(root))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # tests.synth of this tree
import torch  # noqa: E402

import psld_amd  # noqa: E402
from psld_amd import config as C, ops, score_routes as R  # noqa: E402
from psld_amd.registry import get_module  # noqa: E402
from tests.synth import synth_inputs, synth_state_dict  # noqa: E402

what = sys.argv[2]
DEV = "cuda"
assert os.path.abspath(psld_amd.__file__).startswith(os.path.abspath(root)), psld_amd.__file__
wino4 = len(sys.argv) > 3 and sys.argv[3] == "wino4"
if wino4:
    ops.set_winograd_4x4(1)


def cfg_ablation():
    c = C.yaml_default()
    sf = c.model.score_fn
    sf.in_ch, sf.out_ch, sf.nf, sf.ch_mult, sf.num_res_blocks, sf.attn_resolutions, sf.dropout = 6, 6, 128, [1, 2, 2, 2], 2, [16], 0.1
    sde = c.model.sde
    sde.nu, sde.gamma, sde.kappa, sde.decomp_mode = 4.02, 0.02, 0.04, "lower"
    return c


def cfg_vpsde():
    c = C.yaml_default()
    sf = c.model.score_fn
    sf.in_ch, sf.out_ch, sf.nf, sf.ch_mult, sf.num_res_blocks, sf.attn_resolutions, sf.dropout = 3, 3, 128, [1, 2, 2, 2], 4, [16], 0.1
    c.model.sde = C.Config({"name": "vpsde", "beta_min": 0.1, "beta_max": 20.0, "n_timesteps": 1000, "is_augmented": False})
    c.training.loss.name = "score_loss"
    return c


def timed(run, warm, iters):
    """ms per call."""
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


if what == "nets":
    psld_amd.import_modules_into_registry()
    rows = []
    for name, cfg in (("c10_ablation", cfg_ablation()), ("c10_vpsde", cfg_vpsde())):
        vp = cfg.model.sde.name == "vpsde"
        net = get_module("score_fn", "ncsnpp")(cfg)
        net.load_state_dict(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7000))
        net = net.to(DEV)
        sde = get_module("sde", cfg.model.sde.name)(cfg)
        crit = get_module("losses", cfg.training.loss.name)(cfg, sde)
        ch = cfg.model.score_fn.in_ch
        for B in (32, 128):
            x0, eps, t = synth_inputs(B, 3, 32, seed=5)
            if vp:
                eps = eps[:, :3]
            x0, eps, t = x0.to(DEV), eps.contiguous().to(DEV), t.to(DEV)
            net.train()

            def train_step():
                net.zero_grad(set_to_none=False)
                crit(x0, t, net, eps=eps).backward()
            train_ms = timed(train_step, 5, 40)
            net.eval()
            x = torch.randn(B, ch, 32, 32, device=DEV)
            te = torch.rand(B, device=DEV) * 0.9 + 0.05

            def fwd():
                with torch.no_grad():
                    net(x, te)
            fwd_ms = timed(fwd, 5, 60)
            sampler = get_module("samplers", "em_sde")(cfg, sde, net)
            x64 = x.double()
            x32 = x.clone()

            def em_step():              # one predictor update of EulerMaruyamaSampler.sample
                with torch.no_grad():
                    sampler._step(x64, x32, 0.5, 1e-3, torch.randn_like(x64))
            em_ms = timed(em_step, 5, 60)
            rows.append({"net": name, "B": B, "train_ms": round(train_ms, 3), "em_ms": round(em_ms, 3), "fwd_ms": round(fwd_ms, 3)})
        del net
    print(json.dumps({"tree": root, "what": "nets", "wino4": wino4, "rows": rows}), flush=True)
else:
    S = 4
    rows = []
    tiny_a, tiny_o = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    floor = timed(lambda: ops.axpby(tiny_a, 2.0, None, 0.0, tiny_o), 20, 200)
    for c1, c2 in ((256, 0), (256, 256)):
        co, cin = 256, c1 + c2
        for B in ((int(sys.argv[3]),) if len(sys.argv) > 3 else (8, 16, 32, 64, 128)):
            x = torch.randn(B, S, S, cin, device=DEV)           # the tile engine reads the materialised concatenation
            x1 = x[..., :c1].contiguous()
            x2 = x[..., c1:].contiguous() if c2 else None
            dy = torch.randn(B, S, S, co, device=DEV)
            w = torch.randn(co, cin, 3, 3, device=DEV) * 0.05
            y, dx, dw = torch.empty(B, S, S, co, device=DEV), torch.empty(B, S, S, cin, device=DEV), torch.empty_like(w)
            w_fwd = w.permute(0, 2, 3, 1).contiguous()                                   # OHWI
            w_bwd = w.flip(2, 3).transpose(0, 1).permute(0, 2, 3, 1).contiguous()        # rotated, roles swapped
            bias = torch.randn(co, device=DEV)
            epi = ops.epilogue(bias=bias)
            n = co * 9 * cin
            nsplit = R._pick_nsplit(-(-co // 128) * -(-cin // 128) * 9, B * S * S)
            slabs = torch.empty(nsplit * n, device=DEV)

            def tile_wgrad():
                ops.conv2d_wgrad_nhwc(dy, co, x, 3, 3, 1, 1, S, S, slabs, cin, 0, nsplit)
                ops.reduce_slabs(slabs, nsplit, n, dw, layout=1, cout=co, taps=9, cin=cin)
            res = {"tile": {
                "fwd": timed(lambda: ops.conv2d_nhwc(x, None, w_fwd, co, 3, 3, 1, 1, 1, S, S, y, epi), 5, 50),
                "dgrad": timed(lambda: ops.conv2d_nhwc(dy, None, w_bwd, cin, 3, 3, 1, 1, 1, S, S, dx, None), 5, 50),
                "wgrad": timed(tile_wgrad, 5, 50)}}
            if ops.conv3x3_wino_supported(c1, c2, B, S, S, co):
                uf, ub = ops.conv3x3_wino_frag(w, False), ops.conv3x3_wino_frag(w, True)
                res["wino"] = {
                    "fwd": timed(lambda: ops.conv3x3_wino(x1, x2, uf, co, y, epi, allow_split=True), 5, 50),
                    # (a two-source block runs one data gradient per source on slices of these fragments; timed as one launch)
                    "dgrad": timed(lambda: ops.conv3x3_wino(dy, None, ub, cin, dx, None, allow_split=True), 5, 50)}
                if ops.conv3x3_wgrad_wino_supported(co, c1, c2, B, S, S):
                    res["wino"]["wgrad"] = timed(lambda: ops.conv3x3_wgrad_wino(dy, co, x1, dw, x2=x2), 5, 50)
            rows.append({"c1": c1, "c2": c2, "co": co, "B": B,
                         **{k: {d: round(v * 1e3, 1) for d, v in r.items()} for k, r in res.items()}})
    print(json.dumps({"tree": root, "what": "launches", "unit": "us", "floor": round(floor * 1e3, 1), "rows": rows}), flush=True)
