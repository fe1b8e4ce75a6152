"""Record f16 (``--train-math f16``) on the GPU: the fp16 data-gradient fragments, the Winograd and pointwise data gradients with
their operand shift against the CPU reference of the arithmetic (tests/f16_train_ref.py, fp64 accumulation: the kernels differ
from it in fp32 summation order only, the project's 3e-6 kernel gate), ``*_f16s`` with shift 0 against ``*_f16`` bit for bit,
guard-band runs of the new entry points, and a 128-channel network trained under the setting: gradients against the fp32 oracle
within 1.25 x the CPU figure of the same arithmetic (tests/golden/f16_train_meta.json - NOT the 1e-4 parity contract, which
this mode is outside of by design), overfitting, weight caches, the captured training step.  Every test restores the process's
settings."""
import contextlib
import copy
import json
import os

import numpy as np
import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import config as C
from tests import f16_ref as F16
from tests import f16_train_ref as FT
from tests import guard as G
from tests.synth import synth_inputs, synth_state_dict
from tests.test_afhq160_gpu import _leave_the_stream_pool_where_it_was  # noqa: F401  (autouse: the networks built here take streams)
from tests.test_bounds_gpu import guard, pool  # noqa: F401  (fixtures)
from tests.test_kernels_gpu import _nhwc, gen, ops, rel_l2  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
META = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16_train_meta.json")
PAD = 16384         # read-ahead pad of the Winograd fragments
# the two operand scalings of every data-gradient test: dy ~ N(0, 1) with shift 0, dy ~ N(0, 1) * 2^-20 with shift 20
SCALINGS = [(1.0, 0), (2.0 ** -20, 20)]


@contextlib.contextmanager
def record_math(record, mode="bf16x6", winograd=2, wgrad=2, f16=False, shift=None):
    """Record math ``record`` (``f16``: with record f16 on, ``shift``: ops.set_grad_shift) under math mode ``mode`` with
    Winograd forward / data gradient / weight gradient forced."""
    from psld_amd import ops as o
    old, old_r, old_f, old_s = o.math_mode(), o.record_math(), o.record_f16(), o.grad_shift_setting()
    try:
        o.set_math_mode(mode)
        o.set_record_math(record)
        o.set_record_f16(f16)
        o.set_grad_shift(shift)
        o.set_winograd(winograd)
        o.set_wgrad_winograd(wgrad)
        yield
    finally:
        o.set_winograd(None)
        o.set_wgrad_winograd(None)
        o.set_grad_shift(old_s)
        o.set_loss_divisor(None)
        o.set_record_f16(old_f)
        o.set_record_math(old_r)
        o.set_math_mode(old)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# fragments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("co,ci", [(256, 128), (320, 160), (256, 384)])
def test_wino_dgrad_packer_planes(ops, co, ci):
    """psld_pack_conv3x3_wino_dgrad_f16 writes what the batched packer writes for a data-gradient row of its table (the row
    carries the strides and the flip), next to a forward row in the same launch; the payload differs from the forward one."""
    w = gen(co, ci, 3, 3, seed=11, scale=0.05).to(DEV)
    fd, ff = ops.conv3x3_wino_dgrad_frag_f16(w), ops.conv3x3_wino_frag_f16(w)
    payload = co * ci * 32
    assert fd.numel() == ops.conv3x3_wino_frag_bytes_f16(ci, co) == payload + PAD
    outs = [torch.zeros_like(fd), torch.zeros_like(ff)]
    rows = [ops.conv3x3_wino_frag_entry(w, True, outs[0]) + [0], ops.conv3x3_wino_frag_entry(w, False, outs[1]) + [co * ci // 8]]
    ops.pack_wino_batch_f16(torch.tensor(rows, dtype=torch.int64, device=DEV), 2, 2 * (co * ci // 8))
    assert torch.equal(outs[0][:payload], fd[:payload])
    assert torch.equal(outs[1][:payload], ff[:payload])
    assert not torch.equal(fd[:payload], ff[:payload])
    # the same fp16 values as the forward fragments of the transposed, rotated weights (fp32 transform, one rounding)
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    assert torch.equal(fd[:payload], ops.conv3x3_wino_frag_f16(wt)[:payload])


# ---------------------------------------------------------------------------------------------------------------------
# Winograd data gradient
# ---------------------------------------------------------------------------------------------------------------------
def _dgrad_case(ops, co, ci, b, s, scale, shift, seed=40):
    wt = gen(co, ci, 3, 3, seed=seed + 1, scale=0.05)
    dyt = gen(b, co, s, s, seed=seed) * scale
    emu = FT.f16s_dgrad3x3(dyt, wt, shift)
    return wt, dyt, emu, _nhwc(dyt).to(DEV), ops.conv3x3_wino_dgrad_frag_f16(wt.to(DEV))


@pytest.mark.parametrize("scale,shift", SCALINGS, ids=["unit-s0", "2^-20-s20"])
@pytest.mark.parametrize("co,ci,b,s", [(256, 128, 4, 16), (320, 160, 2, 16), (256, 256, 2, 8)],
                         ids=["plain", "tail", "split-chunks"])
def test_conv3x3_dgrad_f16s(ops, co, ci, b, s, scale, shift):
    """dx = conv3x3_wino_f16s(dy, data-gradient fragments, shift): plain launch, channel tail (ci = 160) and split chunks (an 8x8
    map at B = 2: 2 x 2 tiles for 256 CUs) against the reference within 3e-6; repeats bit for bit; alpha and accumulation go
    through the epilogue that carries 2^-shift."""
    wt, dyt, emu, dy, fd = _dgrad_case(ops, co, ci, b, s, scale, shift)
    if (co, ci, b, s) == (256, 256, 2, 8):
        assert ops.conv3x3_wino_ws_bytes(co, 0, b, s, s, ci) > 0           # the split-chunk form really is taken

    def run(e, init):
        y = init.clone()
        ops.conv3x3_wino_f16s(dy, None, fd, ci, y, shift, e, allow_split=True)
        return y
    nan = _nan(b, s, s, ci)
    y = run(None, nan)
    x64 = torch.zeros(b, ci, s, s, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x64, wt.double(), padding=1).backward(dyt.double())
    e_emu, e_64, emu_64 = rel_l2(y.permute(0, 3, 1, 2), emu), rel_l2(y.permute(0, 3, 1, 2), x64.grad), rel_l2(emu, x64.grad)
    print(f"dgrad f16s {b}x{co}->{ci}@{s} scale {scale:g} shift {shift}: vs reference {e_emu:.2e}, vs fp64 {e_64:.2e} "
          f"(reference vs fp64 {emu_64:.2e})")
    assert e_emu <= 3e-6
    assert 0.5 * emu_64 < e_64 < 2 * emu_64 and e_64 > 1e-4         # fp16's 11 bits, not limbs
    assert torch.equal(y, run(None, nan))
    # alpha = 1/2 on top of 2^-shift, accumulated onto zeros: every step exact, so half the plain result bit for bit
    assert torch.equal(run(ops.epilogue(alpha=0.5, accumulate=True), torch.zeros_like(nan)), 0.5 * y)


def test_unshifted_small_gradients_lose_their_bits(ops):
    """dy ~ N(0, 1) * 2^-20 through the launch with shift 0: it computes what the reference with shift 0 computes (dy among
    fp16's subnormals), at least 10 x farther from fp64 than with shift 20 - the shift is what keeps the mode usable."""
    co, ci, b, s = 256, 128, 4, 16
    wt, dyt, emu20, dy, fd = _dgrad_case(ops, co, ci, b, s, 2.0 ** -20, 20)
    emu0 = FT.f16s_dgrad3x3(dyt, wt, 0)
    x64 = torch.zeros(b, ci, s, s, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x64, wt.double(), padding=1).backward(dyt.double())
    ys = {}
    for shift in (0, 20):
        ys[shift] = _nan(b, s, s, ci)
        ops.conv3x3_wino_f16s(dy, None, fd, ci, ys[shift], shift)
    e0, e20 = rel_l2(ys[0].permute(0, 3, 1, 2), x64.grad), rel_l2(ys[20].permute(0, 3, 1, 2), x64.grad)
    print(f"dy ~ 2^-20: shift 0 {e0:.3e} vs fp64, shift 20 {e20:.3e}; launch vs reference at shift 0: "
          f"{rel_l2(ys[0].permute(0, 3, 1, 2), emu0):.2e}")
    assert rel_l2(ys[0].permute(0, 3, 1, 2), emu0) <= 3e-6
    assert e0 >= 10 * e20


@pytest.mark.parametrize("scale,shift", SCALINGS, ids=["unit-s0", "2^-20-s20"])
def test_conv3x3_dgrad_f16s_per_source_slices(ops, scale, shift):
    """One source's share of the data gradient of a convolution that reads a 256 + 128 concatenation: a contiguous slice of the
    fp16 fragments (ordered by 16-channel block of dx), as _resblock_cat_bwd cuts them."""
    b, s, co, c1, c2 = 2, 16, 256, 256, 128
    ci = c1 + c2
    wt, dyt, emu, dy, fd = _dgrad_case(ops, co, ci, b, s, scale, shift, seed=43)
    cut = (fd.numel() - PAD) * c1 // ci
    whole = _nan(b, s, s, ci)
    ops.conv3x3_wino_f16s(dy, None, fd, ci, whole, shift)
    assert rel_l2(whole.permute(0, 3, 1, 2), emu) <= 3e-6
    for lo, hi, fr in ((0, c1, fd[:cut]), (c1, ci, fd[cut:])):
        part = _nan(b, s, s, hi - lo)
        ops.conv3x3_wino_f16s(dy, None, fr, hi - lo, part, shift)
        assert torch.equal(part, whole[..., lo:hi])          # a channel's result does not depend on who shares its launch
        # as the executor launches it: split chunks where the grid is small (another summation order: the gate, and repeatable)
        split, again = _nan(b, s, s, hi - lo), _nan(b, s, s, hi - lo)
        ops.conv3x3_wino_f16s(dy, None, fr, hi - lo, split, shift, allow_split=True)
        ops.conv3x3_wino_f16s(dy, None, fr, hi - lo, again, shift, allow_split=True)
        err = rel_l2(split.permute(0, 3, 1, 2), emu[:, lo:hi])
        print(f"dgrad f16s source [{lo}:{hi}] of {ci}, shift {shift}: {err:.2e}")
        assert err <= 3e-6 and torch.equal(split, again)


# ---------------------------------------------------------------------------------------------------------------------
# pointwise data gradient
# ---------------------------------------------------------------------------------------------------------------------
M_PW = 16384


def _pw_check(ops, tag, dyt, wt_nk, frag, width, shift, col0=0):
    """dx[m][width] = dy[m][k] W[k][n] columns col0 .. col0 + width on ``frag`` against the reference."""
    m = dyt.shape[0]
    emu = FT.f16s_matmul_dgrad(dyt, wt_nk, shift)[:, col0:col0 + width]
    ref64 = (dyt.double() @ wt_nk.double())[:, col0:col0 + width]
    dy = dyt.to(DEV)

    def run(e, init):
        y = init.clone()
        ops.gemm_split_f16s(dy, None, m, frag, width, y, shift, e)
        return y
    nan = _nan(m, width)
    y = run(None, nan)
    e_emu, e_64 = rel_l2(y, emu), rel_l2(y, ref64)
    print(f"{tag}, shift {shift}: vs reference {e_emu:.2e}, vs fp64 {e_64:.2e} (reference vs fp64 {rel_l2(emu, ref64):.2e})")
    assert e_emu <= 3e-6
    assert e_64 > 1e-4
    assert torch.equal(y, run(None, nan))
    return y


@pytest.mark.parametrize("scale,shift", SCALINGS, ids=["unit-s0", "2^-20-s20"])
def test_pointwise_dgrad_f16s(ops, scale, shift):
    """256 -> 256 at m = 16384 (128 tiles: the smallest launch the policy gives to the kernel), and a ``cols`` slice of 512 -> 256:
    the second 256 input channels of a 1x1 weight stored [256 out][512 in] from the second half of its fragments."""
    m = M_PW
    dyt = gen(m, 256, seed=50) * scale
    assert ops.gemm_split_f16_wanted(256, 0, m, 256) and not ops.gemm_split_f16_wanted(256, 0, m - 128, 256)
    w1 = gen(256, 256, seed=51, scale=0.05)                 # [out = k of the data gradient][in = n]
    f1 = ops.gemm_frag_f16(w1.to(DEV), 256, 256, 1, 256)
    _pw_check(ops, "pointwise dgrad f16s 256->256", dyt, w1, f1, 256, shift)
    w2 = gen(256, 512, seed=52, scale=0.05)
    f2 = ops.gemm_frag_f16(w2.to(DEV), 512, 256, 1, 512)
    whole = _pw_check(ops, "pointwise dgrad f16s 256->512", dyt, w2, f2, 512, shift)
    part = _pw_check(ops, "pointwise dgrad f16s 256->512, columns 256:512", dyt, w2, f2[f2.numel() // 2:], 256, shift, col0=256)
    assert torch.equal(part, whole[:, 256:])


def _attention_harness(c, seed=78):
    from psld_amd import score_fn as S
    from tests.test_blocks_gpu import Harness
    mod = S.AttnBlockpp(c)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in mod.state_dict().items()], seed)
    return Harness(mod, sd), sd


@pytest.mark.parametrize("scale,shift", SCALINGS, ids=["unit-s0", "2^-20-s20"])
def test_qkv_data_gradient_set_f16s(ops, scale, shift):
    """The shared q | k | v data-gradient set of an attention block at c = 256 as the executor builds it (three parameters
    placed along K = 3c by the batched packer's chunk placement, entries 'qkv_d_f16' under the holder 'qkv_set_d_f16'): it equals
    the fp16 fragments of the concatenated matrix, the launch meets the gate, and the batched refresh of the 'limb_f16' family
    fills it anew after the weights moved."""
    c, m = 256, M_PW
    with record_math("bf16x3", f16=True):
        h, _ = _attention_harness(c)
        net, mod = h.net, h.mod
        nins = (mod.NIN_0, mod.NIN_1, mod.NIN_2)

        def sets():
            wcat = torch.cat([n_.W.detach() for n_ in nins], dim=1).contiguous()     # B[n = c in][k = 3c out]
            pd = net._qkv_frags_x3(mod, True, f16=True)
            assert torch.equal(pd, ops.gemm_frag_f16(wcat, c, 3 * c, 3 * c, 1))
            return wcat, pd
        wcat, pd = sets()
        dt = gen(m, 3 * c, seed=60) * scale
        _pw_check(ops, "q|k|v data gradient f16s 768->256", dt, wcat.cpu().t().contiguous(), pd, c, shift)
        before, ptr = pd.clone(), pd.data_ptr()
        tags = {tag for _, tag in net._wcache.entries}
        assert {"qkv_set_d_f16", "qkv_d_f16"} <= tags, sorted(tags)
        with torch.no_grad():
            for i, n_ in enumerate(nins):
                n_.W.add_(gen(c, c, seed=61 + i, scale=0.02).to(DEV))
        net.weights_changed()
        wcat_b, pd_b = sets()
        assert pd_b.data_ptr() == ptr and not torch.equal(pd_b, before) and not torch.equal(wcat_b, wcat)


# ---------------------------------------------------------------------------------------------------------------------
# shift 0 is the unshifted entry, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def test_f16s_with_shift_0_is_f16_bitwise(ops):
    """Forward shapes: Winograd 256 -> 256 @16 at B = 4 and pointwise 512 -> 256 at m = 16384, plain and with a full epilogue."""
    b, s, c = 4, 16, 256
    x = _nhwc(gen(b, c, s, s, seed=1)).to(DEV)
    ff = ops.conv3x3_wino_frag_f16(gen(c, c, 3, 3, seed=2, scale=0.05).to(DEV))
    bias, res = gen(c, seed=3).to(DEV), _nhwc(gen(b, c, s, s, seed=4)).to(DEV)
    for mk in (lambda: None, lambda: ops.epilogue(alpha=0.7, bias=bias, residual=res, ld_residual=c, out_scale=0.5)):
        ya, yb = _nan(b, s, s, c), _nan(b, s, s, c)
        ops.conv3x3_wino_f16(x, None, ff, c, ya, mk(), allow_split=True)
        ops.conv3x3_wino_f16s(x, None, ff, c, yb, 0, mk(), allow_split=True)
        assert torch.equal(ya, yb) and bool(torch.isfinite(ya).all())
    m, k, n = M_PW, 512, 256
    a = gen(m, k, seed=5).to(DEV)
    fp = ops.gemm_frag_f16(gen(n, k, seed=6, scale=0.05).to(DEV), n, k, k, 1)
    pb, pr = gen(n, seed=7).to(DEV), gen(m, n, seed=8).to(DEV)
    for mk in (lambda: None, lambda: ops.epilogue(alpha=0.7, bias=pb, residual=pr, ld_residual=n, out_scale=0.5)):
        ya, yb = _nan(m, n), _nan(m, n)
        ops.gemm_split_f16(a, None, m, fp, n, ya, mk())
        ops.gemm_split_f16s(a, None, m, fp, n, yb, 0, mk())
        assert torch.equal(ya, yb) and bool(torch.isfinite(ya).all())
    # two sources through the shifted entry as well
    ya, yb = _nan(m, n), _nan(m, n)
    ops.gemm_split_f16(a[:, :256].contiguous(), a[:, 256:].contiguous(), m, fp, n, ya, None)
    ops.gemm_split_f16s(a[:, :256].contiguous(), a[:, 256:].contiguous(), m, fp, n, yb, 0, None)
    assert torch.equal(ya, yb)


def test_shift_outside_its_range_is_refused(ops):
    x, y = _nhwc(gen(1, 128, 8, 8, seed=1)).to(DEV), _nan(1, 8, 8, 128)
    ff = ops.conv3x3_wino_frag_f16(gen(128, 128, 3, 3, seed=2).to(DEV))
    for bad in (-1, 25):
        with pytest.raises(RuntimeError, match="shift"):
            ops.conv3x3_wino_f16s(x, None, ff, 128, y, bad)
    a, yp = gen(M_PW, 256, seed=3).to(DEV), _nan(M_PW, 256)
    fp = ops.gemm_frag_f16(gen(256, 256, seed=4).to(DEV), 256, 256, 256, 1)
    for bad in (-1, 25):
        with pytest.raises(RuntimeError, match="shift"):
            ops.gemm_split_f16s(a, None, M_PW, fp, 256, yp, bad)


# ---------------------------------------------------------------------------------------------------------------------
# guard bands (tests/guard.py): the new packer and the four new launch forms on buffers of exactly the documented size
# ---------------------------------------------------------------------------------------------------------------------
def _R(*shape, seed, scale=1.0):
    return gen(*shape, seed=seed, scale=scale).to(DEV)


def _guard_dgrad_pack(co, ci):
    def build(ops):
        t = dict(w=_R(co, ci, 3, 3, seed=3, scale=0.1),
                 out=torch.zeros(ops.conv3x3_wino_frag_bytes_f16(ci, co), dtype=torch.uint8, device=DEV))
        return (lambda w, out: ops.conv3x3_wino_dgrad_frag_f16(w, out)), t, ["out"], 0
    return build


def _guard_dgrad_conv(co, c_lo, c_hi, ci, b, s, shift, min_ws=0):
    """The data gradient's launch on the fragment slice of input channels [c_lo, c_hi) of ``ci``."""
    def build(ops):
        fd = ops.conv3x3_wino_dgrad_frag_f16(_R(co, ci, 3, 3, seed=3, scale=0.1))
        assert c_hi == ci               # the last source's slice ends with the fragments' read-ahead pad
        fr = fd[(fd.numel() - PAD) * c_lo // ci:].clone()
        t = dict(dy=_R(b, s, s, co, seed=40, scale=2.0 ** -shift), fr=fr, dx=_nan(b, s, s, c_hi - c_lo))
        return (lambda dy, fr, dx: ops.conv3x3_wino_f16s(dy, None, fr, c_hi - c_lo, dx, shift, None, allow_split=True)), t, ["dx"], min_ws
    return build


def _guard_pw_dgrad(m, k, n, lo, hi, shift):
    def build(ops):
        f = ops.gemm_frag_f16(_R(k, n, seed=51, scale=0.05), n, k, 1, n)
        fr = f[f.numel() * lo // n:f.numel() * hi // n].clone()
        t = dict(dy=_R(m, k, seed=50, scale=2.0 ** -shift), fr=fr, dx=_R(m, hi - lo, seed=52))
        return (lambda dy, fr, dx: ops.gemm_split_f16s(dy, None, m, fr, hi - lo, dx, shift,
                                                       ops.epilogue(alpha=0.5, accumulate=True))), t, ["dx"], 0
    return build


GUARDED = {
    "pack-wino_dgrad_f16-256x128": _guard_dgrad_pack(256, 128),
    "pack-wino_dgrad_f16-320x160": _guard_dgrad_pack(320, 160),
    "dgrad_f16s-plain-4x256->128@16": _guard_dgrad_conv(256, 0, 128, 128, 4, 16, 20),
    "dgrad_f16s-tail-2x320->160@16": _guard_dgrad_conv(320, 0, 160, 160, 2, 16, 0),
    "dgrad_f16s-split-2x256->256@8": _guard_dgrad_conv(256, 0, 256, 256, 2, 8, 20, min_ws=1),
    "dgrad_f16s-slice-2x256->[256:384]@16": _guard_dgrad_conv(256, 256, 384, 384, 2, 16, 20),
    "pw_dgrad_f16s-256->512": _guard_pw_dgrad(M_PW, 256, 512, 0, 512, 20),
    "pw_dgrad_f16s-256->512[256:512]": _guard_pw_dgrad(M_PW, 256, 512, 256, 512, 0),
}


@pytest.mark.parametrize("name", list(GUARDED))
def test_bounds_of_the_fp16_training_launches(ops, guard, name):
    fn, tensors, outputs, min_ws = GUARDED[name](ops)
    torch.cuda.synchronize()
    G.run_guarded(guard, fn, tensors, outputs)
    assert guard.workspace_calls >= min_ws, f"{guard.workspace_calls} guarded workspace calls, expected {min_ws}"


# ---------------------------------------------------------------------------------------------------------------------
# network
# ---------------------------------------------------------------------------------------------------------------------
F16_LAUNCHES = ("conv3x3_wino_f16", "conv3x3_wino_f16s", "gemm_split_f16", "gemm_split_f16s")
OTHER_WINO = ("conv3x3_wino", "conv3x3_wino_x3")


def _tiny128(attn=True):
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    cfg = C.tiny(nf=128, ch_mult=(1, 1), attn_resolutions=(16,) if attn else (8,))
    sde = get_module("sde", "psld")(cfg)
    return cfg, sde, get_module


def test_tiny_network_gradients_under_record_f16(monkeypatch):
    """C.tiny(nf=128, ch_mult=(1, 1)) at B = 2, 16x16, the fixture's network and inputs, under ``--train-math f16``'s settings
    with Winograd forced: all parameter gradients against the fp32 oracle within 1.25 x the fixture's figure for the same
    arithmetic (the GPU leaves some launches on limbs, so at or below it; 25 % for rounding decisions that flip with the
    summation order), the loss within 1e-2 relative; the backward pass ran the shifted fp16 launches with the automatic shift
    (12 for 3072 elements) and no Winograd launch on limbs; with the flag off again the gradients are bitwise those computed
    before it was switched on."""
    from psld_amd import ops as o
    from psld_amd.registry import get_module
    import psld_amd
    psld_amd.import_modules_into_registry()
    with open(META) as fh:
        meta = json.load(fh)["tiny128"]
    cfg = C.tiny(nf=128, ch_mult=(1, 1))
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    x0, eps, t = synth_inputs(2, 3, 16, seed=3)

    def grads(f16, log=None):
        for p in net.parameters():
            p.grad = None
        with record_math("bf16x3", f16=f16):
            if log is not None:
                for name in F16_LAUNCHES + OTHER_WINO:
                    def rec(*a, _fn=getattr(o, name), _name=name, **k):
                        log.append((_name, a[5] if _name == "conv3x3_wino_f16s" else a[6] if _name == "gemm_split_f16s" else None))
                        return _fn(*a, **k)
                    monkeypatch.setattr(o, name, rec)
            loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
            loss.backward()
            if log is not None:
                monkeypatch.undo()
        return loss.item(), net.flat_grad().clone()
    _, g_before = grads(False)
    log = []
    loss, g16 = grads(True, log)
    grads16 = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}
    _, g_after = grads(False)
    assert torch.equal(g_before, g_after) and not torch.equal(g16, g_before)
    names = {n for n, _ in log}
    print("launches under record f16:", {k: sum(1 for n, _ in log if n == k) for k in sorted(names)})
    assert {"conv3x3_wino_f16", "conv3x3_wino_f16s"} <= names and not names & set(OTHER_WINO)
    assert {s for n, s in log if n.endswith("f16s")} == {meta["shift_auto"]} == {12}
    osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
    oloss = O.psld_score_loss(O.PSLDOracle.from_config(cfg), x0, t, lambda z, tt: O.ncsnpp_forward(osd, cfg, z, tt), eps)
    oloss.backward()
    ref = {k: v.grad for k, v in osd.items() if v.grad is not None}
    assert grads16.keys() == ref.keys()
    num = torch.stack([(grads16[k].double() - ref[k].double()).norm() for k in ref]).norm().item()
    den = torch.stack([ref[k].double().norm() for k in ref]).norm().item()
    print(f"tiny nf=128 under record f16: loss {loss:.6f} (oracle {oloss.item():.6f}); gradients global rel-L2 {num / den:.3e} "
          f"(CPU oracle, same arithmetic: {meta['auto']['grads_rel_l2']:.3e}; two limbs {meta['two_limb_grads_rel_l2']:.3e})")
    assert num / den <= 1.25 * meta["auto"]["grads_rel_l2"]
    assert abs(loss - oloss.item()) <= 1e-2 * abs(oloss.item())


def test_c10_gradients_with_every_fp16_launch_under_record_f16(monkeypatch):
    """C10-SOTA at B = 2 on the fixture's weights and inputs, Winograd forced and the pointwise policy widened to every shape the
    eight-wave kernel takes (at B = 2 the 128-tile threshold would leave all of them on limbs): the executor's pointwise forward
    and data-gradient launches - 1x1 shortcuts with their per-source column slices, NIN projections, the q | k | v set, the input
    pyramid - run on fp16 next to the Winograd ones, from the 'fwd_f16' / 'dgrad_f16' / 'qkv_d_f16' / 'wfrag_d_f16' cache entries.
    All parameter gradients against the fp32 oracle within 1.25 x the fixture's figure for this network."""
    import os as _os
    from psld_amd import ops as o
    from psld_amd.registry import get_module
    import psld_amd
    psld_amd.import_modules_into_registry()
    with open(META) as fh:
        meta = json.load(fh)["c10_sota"]
    cfg = C.c10_sota()
    cfg.model.score_fn.dropout = 0.0
    sde = get_module("sde", "psld")(cfg)
    crit = get_module("losses", "psld_score_loss")(cfg, sde)
    net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    net.sf.dropout = 0.0
    x0, eps, t = synth_inputs(2, 3, 32, seed=3)
    log = []
    with record_math("bf16x3", f16=True):
        monkeypatch.setattr(o, "gemm_split_f16_wanted", o.gemm_split_f16_supported)
        for name in F16_LAUNCHES + OTHER_WINO + ("gemm_split_x3",):
            def rec(*a, _fn=getattr(o, name), _name=name, **k):
                log.append((_name, a[5] if _name == "conv3x3_wino_f16s" else a[6] if _name == "gemm_split_f16s" else None))
                return _fn(*a, **k)
            monkeypatch.setattr(o, name, rec)
        loss = crit(x0.to(DEV), t.to(DEV), net, eps=eps.to(DEV))
        loss.backward()
        monkeypatch.undo()
        tags = {tag for _, tag in net._wcache.entries}
    names = {n for n, _ in log}
    print("launches:", {k: sum(1 for n, _ in log if n == k) for k in sorted(names)})
    assert set(F16_LAUNCHES) <= names and not names & set(OTHER_WINO)
    assert {s for n, s in log if n.endswith("f16s")} == {meta["shift_auto"]} == {14}
    assert {"wfrag_f16", "wfrag_d_f16", "fwd_f16", "dgrad_f16", "qkv_set_d_f16", "qkv_d_f16"} <= tags, sorted(tags)
    grads16 = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, _os.cpu_count() or 1)))
    try:
        osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
        oloss = O.psld_score_loss(O.PSLDOracle.from_config(cfg), x0, t, lambda z, tt: O.ncsnpp_forward(osd, cfg, z, tt), eps)
        oloss.backward()
    finally:
        torch.set_num_threads(threads)
    ref = {k: v.grad for k, v in osd.items() if v.grad is not None}
    assert grads16.keys() == ref.keys()
    num = torch.stack([(grads16[k].double() - ref[k].double()).norm() for k in ref]).norm().item()
    den = torch.stack([ref[k].double().norm() for k in ref]).norm().item()
    print(f"c10_sota B=2 under record f16, every fp16 launch: loss {loss.item():.6f} (oracle {oloss.item():.6f}); gradients global "
          f"rel-L2 {num / den:.3e} (CPU oracle, same arithmetic: {meta['auto']['grads_rel_l2']:.3e})")
    assert num / den <= 1.25 * meta["auto"]["grads_rel_l2"]
    assert abs(loss.item() - oloss.item()) <= 1e-2 * abs(oloss.item())


def test_training_overfits_fixed_batch_under_record_f16():
    """150 steps on one fixed batch (test_training_overfits_fixed_batch_under_record_math's recipe) on the 128-channel tiny
    network with attention on its 16x16 maps: the last loss below half the first."""
    from psld_amd.optim import FusedAdam
    cfg, sde, get_module = _tiny128()
    x0, eps, t = (v.to(DEV) for v in synth_inputs(8, 3, 16, seed=5))
    with record_math("bf16x3", f16=True):
        torch.manual_seed(0)
        net = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        opt = FusedAdam(net, lr=1e-3, grad_clip=1.0)
        losses = []
        for _ in range(150):
            loss = crit(x0, t, net, eps=eps)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        losses = torch.stack(losses).cpu().numpy()
    assert np.isfinite(losses).all()
    print(f"overfit under record f16, 150 steps: {float(losses[0]):.4f} -> {float(losses[-1]):.3e}")
    assert float(losses[-1]) < 0.5 * float(losses[0])


def test_weight_caches_follow_the_optimizer_under_record_f16():
    """After three optimizer steps with warm fp16 caches (forward and data-gradient fragments refreshed by the batched packers)
    a fresh network loaded with the weights agrees bitwise in the next step's gradients: a step changes the gradients the way a
    fresh pack does."""
    from psld_amd.optim import FusedAdam
    cfg, sde, get_module = _tiny128()
    with record_math("bf16x3", f16=True):
        torch.manual_seed(1)
        net = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        opt = FusedAdam(net, lr=1e-3, grad_clip=1.0)
        x0, eps, t = (v.to(DEV) for v in synth_inputs(4, 3, 16, seed=9))
        crit(x0, t, net, eps=eps).backward()
        g_first = net.flat_grad().clone()
        opt.step()
        for _ in range(2):
            crit(x0, t, net, eps=eps).backward()
            opt.step()
        tags = {tag for _, tag in net._wcache.entries}
        assert {"wfrag_f16", "wfrag_d_f16"} <= tags, sorted(tags)
        fresh = get_module("score_fn", "ncsnpp")(cfg)
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
        fresh = fresh.to(DEV).train()
        for n_ in (net, fresh):
            for p_ in n_.parameters():
                p_.grad = None
        torch.manual_seed(5); crit(x0, t, net, eps=eps).backward()
        torch.manual_seed(5); crit(x0, t, fresh, eps=eps).backward()
        assert torch.equal(net.flat_grad(), fresh.flat_grad())
        assert not torch.equal(net.flat_grad(), g_first)


def test_graph_captured_training_step_under_record_f16():
    """The captured training step under record f16 is bitwise the eager step, and a change of the gradient shift between steps
    captures anew instead of replaying the other shift's launches."""
    from psld_amd.optim import EMAWeightUpdate
    cfg, sde, get_module = _tiny128()
    cfg.model.score_fn.dropout = 0.0
    cfg.training.optimizer.warmup = 4
    torch.manual_seed(3)
    net_a = get_module("score_fn", "ncsnpp")(cfg).to(DEV).train()
    net_b = copy.deepcopy(net_a)
    data = [torch.rand(4, 3, 16, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(i)) * 2 - 1 for i in range(10)]
    # steps 0-4 with the automatic shift (two eager warm-up steps, the capture, two replays), steps 5-9 with --grad-shift 6
    plan = [None] * 5 + [6] * 5
    runs = []
    for net, graphs in ((net_a, False), (net_b, True)):
        ema = copy.deepcopy(net)
        for p in ema.parameters():
            p.requires_grad = False
        crit = get_module("losses", "psld_score_loss")(cfg, sde)
        wr = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema, criterion=crit)
        if graphs:
            wr.enable_graphs(True, warmup_steps=2)
        cb = EMAWeightUpdate(cfg.training.ema_decay)
        torch.manual_seed(11)
        losses = []
        for i, shift in enumerate(plan):
            with record_math("bf16x3", f16=True, shift=shift):
                losses.append(wr.training_step(data[i], i).item())
                cb.on_train_batch_end(None, wr)
        runs.append((losses, net.flatten_parameters().clone(), ema.flatten_parameters().clone()))
        if graphs:
            keys = list(wr._graph_steps)
            assert len(keys) == 2 and {k[4] for k in keys} == {None, 6} and all(k[3] == ("f16", "x3", "x6") for k in keys), keys
            assert all("graph" in e for e in wr._graph_steps.values())
    (la, pa, ea), (lb, pb, eb) = runs
    print("eager  losses", la)
    print("graph  losses", lb)
    assert la == lb and torch.equal(pa, pb) and torch.equal(ea, eb)
