"""Record f16 (``--train-math f16``: one fp16 product in the forward and data-gradient launches of a recording pass) - what can
be checked without a GPU: the setting in the C ABI, Python and the environment, the CLI options, the gradient-shift rule and its
host state, and the CPU reference of the arithmetic (tests/f16_train_ref.py) against fp64 autograd and, routed through the
oracle, against the fp32 oracle and the recorded figures of tests/golden/f16_train_meta.json."""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import psld_oracle as O
from psld_amd import _lib, config as C
from tests import f16_train_ref as FT
from tests import x3_train_ref as XT
from tests.synth import synth_inputs, synth_state_dict
from tests.test_oracle_golden import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = os.path.join(ROOT, "tests", "golden", "f16_train_meta.json")


def test_record_f16_setter_and_getter():
    from psld_amd import ops
    lib = _lib.load()
    before = lib.psld_get_record_f16()
    others = (lib.psld_get_math_mode(), lib.psld_get_record_math(), lib.psld_get_eval_math())
    try:
        assert lib.psld_set_record_f16(1) == 0 and lib.psld_get_record_f16() == 1 and ops.record_f16() is True
        for bad in (2, -1, 3):
            assert lib.psld_set_record_f16(bad) != 0 and b"psld_set_record_f16" in lib.psld_last_error()
            assert lib.psld_get_record_f16() == 1
        assert lib.psld_set_record_f16(0) == 0 and ops.record_f16() is False
        ops.set_record_f16(True)
        assert lib.psld_get_record_f16() == 1
        with pytest.raises(ValueError):
            ops.set_record_f16(2)
        with pytest.raises(ValueError):
            ops.set_record_f16("f16")
        assert ops.record_f16() is True
    finally:
        lib.psld_set_record_f16(before)
    assert lib.psld_version() == _lib.ABI_VERSION == 14
    assert others == (lib.psld_get_math_mode(), lib.psld_get_record_math(), lib.psld_get_eval_math())


def test_record_f16_is_independent_of_the_three_other_settings():
    """Each of the four setters moves its own value only; record math still has two values and the math mode three."""
    lib = _lib.load()
    getters = (lib.psld_get_math_mode, lib.psld_get_record_math, lib.psld_get_eval_math, lib.psld_get_record_f16)
    setters = (lib.psld_set_math_mode, lib.psld_set_record_math, lib.psld_set_eval_math, lib.psld_set_record_f16)
    values = ((0, 1, 2), (1, 2), (0, 1), (0, 1))
    before = [g() for g in getters]
    try:
        for i, (setter, vals) in enumerate(zip(setters, values)):
            for v in vals:
                start = [g() for g in getters]
                assert setter(v) == 0
                now = [g() for g in getters]
                assert now[i] == v and now[:i] + now[i + 1:] == start[:i] + start[i + 1:], (i, v, start, now)
        for bad in (0, 3, -1):
            assert lib.psld_set_record_math(bad) != 0       # no new value of record math ...
        assert lib.psld_set_math_mode(3) != 0               # ... nor of the math mode
    finally:
        for setter, v in zip(setters, before):
            setter(v)


@pytest.mark.parametrize("value,expect", [(None, (1, 1, 0, 0)), ("f16_train", (2, 2, 0, 1)), ("bf16x3_train", (2, 2, 0, 0)),
                                          ("f16", (2, 1, 1, 0)), ("f16_training", (1, 1, 0, 0))])
def test_environment_spelling(value, expect):
    """PSLD_MATH=f16_train: math mode bf16x3, record math bf16x3, eval math left at limb, record f16 on - read once per
    process, through either getter first; the other spellings leave record f16 off."""
    env = {k: v for k, v in os.environ.items() if k != "PSLD_MATH"}
    if value is not None:
        env["PSLD_MATH"] = value
    for first in ("lib.psld_get_record_f16()", "lib.psld_get_math_mode()"):
        code = (f"from psld_amd import _lib; lib = _lib.load(); {first}; "
                "print(lib.psld_get_math_mode(), lib.psld_get_record_math(), lib.psld_get_eval_math(), lib.psld_get_record_f16())")
        out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        assert tuple(int(v) for v in out.stdout.split()) == expect, (value, first, out.stdout)


def test_cli_options():
    from psld_amd import cli
    ap = cli.build_parser()
    for cmd in ("train", "train_clf"):
        assert ap.parse_args([cmd, "--train-math", "f16"]).train_math == "f16"
        with pytest.raises(SystemExit):
            ap.parse_args([cmd, "--train-math", "f32"])
    a = ap.parse_args(["train", "--train-math", "f16", "--grad-shift", "20"])
    assert a.train_math == "f16" and a.grad_shift == 20
    assert ap.parse_args(["train"]).grad_shift is None          # default: automatic
    for cmd in ("sample", "cc_sample", "inpaint"):
        with pytest.raises(SystemExit):
            ap.parse_args([cmd, "--train-math", "f16"])
        with pytest.raises(SystemExit):
            ap.parse_args([cmd, "--grad-shift", "3"])


def test_shift_rule_and_its_host_state():
    from psld_amd import ops
    assert ops.grad_shift_for(786432) == 20 and FT.shift_for(786432) == 20       # B = 128 of 2 x 3 x 32 x 32: 1.5 * 2^19
    assert ops.grad_shift_for(1) == 0 and ops.grad_shift_for(None) == 0 and ops.grad_shift_for(0) == 0
    assert ops.grad_shift_for(2) == 1 and ops.grad_shift_for(3072) == 12 and ops.grad_shift_for(4096) == 12
    assert ops.grad_shift_for(4097) == 13 and ops.grad_shift_for(128) == 7
    assert ops.grad_shift_for(2 ** 24) == 24 and ops.grad_shift_for(2 ** 24 + 1) == 24 and ops.grad_shift_for(2 ** 40) == 24
    for n in (1, 2, 3, 1000, 3072, 786432, 2 ** 30):
        assert ops.grad_shift_for(n) == FT.shift_for(n)
    old = ops.grad_shift_setting()
    try:
        ops.set_grad_shift(None)
        ops.set_loss_divisor(None)
        assert ops.take_grad_shift() == 0                   # nobody published a divisor: a user's own loss, the guidance pass
        ops.set_loss_divisor(786432)
        assert ops.current_grad_shift() == 20 and ops.loss_divisor() == 786432
        assert ops.take_grad_shift() == 20 and ops.loss_divisor() is None and ops.take_grad_shift() == 0     # consumed
        for forced, want in ((5, 5), (0, 0), (-3, 0), (99, 24)):
            ops.set_grad_shift(forced)
            ops.set_loss_divisor(786432)
            assert ops.grad_shift_setting() == want and ops.take_grad_shift() == want
    finally:
        ops.set_grad_shift(old)
        ops.set_loss_divisor(None)


def test_losses_publish_their_divisor():
    """The autograd nodes of the three losses publish the divisor of the gradient they hand on when their backward runs (right
    before the network's): the element count for a mean, the batch for the cross-entropy, 1 for a sum."""
    from psld_amd import losses, ops

    class Ctx:
        saved_tensors = (torch.ones(2, 3),)
    try:
        for fn, div, n_out in ((losses._SqErr, 384, 3), (losses._VpScoreLoss, 1, 7)):
            Ctx.divisor = div
            ops.set_loss_divisor(None)
            out = fn.backward(Ctx, torch.tensor(1.0))
            assert len(out) == n_out and ops.loss_divisor() == div
        Ctx.divisor = 16
        losses._SoftmaxXent.backward(Ctx, torch.tensor(1.0), None)
        assert ops.take_grad_shift() == 4
    finally:
        ops.set_loss_divisor(None)


def test_reference_data_gradient_with_and_without_the_shift():
    """One 3x3 layer, dy ~ N(0, 1) * 2^-20 (what a mean over ~10^6 elements hands on): the reference's data gradient with shift 20
    against fp64 autograd sits at fp16's rounding (11 bits), without the shift dy is rounded among the subnormals (spacing 2^-24:
    four bits or fewer) and lies at least 10 x farther away (expected from the spacing: 20-40 x)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 16, 16, generator=g)
    w = torch.randn(96, 64, 3, 3, generator=g) * 0.05
    dy = torch.randn(2, 96, 16, 16, generator=g) * 2.0 ** -20
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    torch.nn.functional.conv2d(x64, w64, padding=1).backward(dy.double())
    e20, e0 = rel_l2(FT.f16s_dgrad3x3(dy, w, 20), x64.grad), rel_l2(FT.f16s_dgrad3x3(dy, w, 0), x64.grad)
    print(f"fp16 data gradient of dy ~ 2^-20 vs fp64: shift 20 {e20:.3e}, shift 0 {e0:.3e}, ratio {e0 / e20:.1f}")
    assert 1e-4 < e20 < 1e-3
    assert e0 >= 10 * e20
    # the shift is exact: the same operand at scale 1 with shift 0 gives the same relative error, bit for bit the same values
    a = FT.f16s_dgrad3x3(dy * 2.0 ** 20, w, 0) * 2.0 ** -20
    assert torch.equal(a, FT.f16s_dgrad3x3(dy, w, 20))
    # weight gradient: x3_train_ref's two-limb one, untouched by the shift
    assert rel_l2(XT.two_limb_wgrad3x3(x, dy), w64.grad) < 2e-5


def test_routed_oracle_on_a_128_channel_net(monkeypatch):
    """The oracle's parameter gradients on C.tiny(nf=128, ch_mult=(1, 1)) at B = 2 under the routed arithmetic against the fp32
    oracle: the figure of the fixture (to 2 %), larger than the two-limb figure (the arithmetic really is narrower), and larger
    again with shift 0."""
    with open(META) as fh:
        meta = json.load(fh)["tiny128"]
    cfg = C.tiny(nf=128, ch_mult=(1, 1))
    from psld_amd.registry import get_module
    import psld_amd
    psld_amd.import_modules_into_registry()
    net = get_module("score_fn", "ncsnpp")(cfg)
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 7)
    x0, eps, t = synth_inputs(2, 3, 16, seed=3)
    sde = O.PSLDOracle.from_config(cfg)

    def run():
        osd = {k: v.clone().requires_grad_(k != "all_modules.0.W") for k, v in sd.items()}
        loss = O.psld_score_loss(sde, x0, t, lambda z, tt: O.ncsnpp_forward(osd, cfg, z, tt), eps)
        loss.backward()
        return loss.detach(), {k: v.grad for k, v in osd.items() if v.grad is not None}

    def dist(g, ref):
        num = torch.stack([(g[k].double() - ref[k].double()).norm() for k in ref]).norm().item()
        return num / torch.stack([ref[k].double().norm() for k in ref]).norm().item()
    l32, g32 = run()
    auto = FT.shift_for(2 * 6 * 16 * 16)
    assert auto == meta["shift_auto"] == 12
    state = FT.route_oracle_autograd(monkeypatch, O, auto)
    la, ga = run()
    state["shift"] = 0
    _, g0 = run()
    monkeypatch.undo()
    XT.route_oracle_autograd(monkeypatch, O)
    _, g2 = run()
    monkeypatch.undo()
    ea, e0, e2 = dist(ga, g32), dist(g0, g32), dist(g2, g32)
    print(f"routed oracle, tiny nf=128: loss {la.item():.6f} vs {l32.item():.6f}; gradients global rel-L2: shift {auto} {ea:.3e} "
          f"(fixture {meta['auto']['grads_rel_l2']:.3e}), shift 0 {e0:.3e} (fixture {meta['shift0']['grads_rel_l2']:.3e}), "
          f"two limbs {e2:.3e}")
    assert abs(ea - meta["auto"]["grads_rel_l2"]) <= 0.02 * meta["auto"]["grads_rel_l2"]
    assert abs(e0 - meta["shift0"]["grads_rel_l2"]) <= 0.02 * meta["shift0"]["grads_rel_l2"]
    assert ea > e2 and e0 > ea
    assert abs(la.item() - l32.item()) < 1e-2 * abs(l32.item())


def test_fixture_census():
    """The recorded census: with the automatic shift nothing is clamped on either network, and the shift - which only moves
    values up - leaves a smaller share of the operands below fp16's normal range and below half its smallest subnormal than
    shift 0 does (no level is asserted: how small a deep site's gradients are is the synthetic weights' doing)."""
    with open(META) as fh:
        meta = json.load(fh)
    assert set(meta) == {"tiny128", "c10_sota"}
    for name, m in meta.items():
        assert m["shift_auto"] == FT.shift_for(m["divisor"])
        ca, c0 = m["auto"]["census"], m["shift0"]["census"]
        assert ca["share_clamped"] == 0.0 and ca["max_abs"] < 65504.0, name
        assert ca["share_below_2m14"] < c0["share_below_2m14"] and ca["share_below_2m25"] < c0["share_below_2m25"], name
        assert ca["sites"] == c0["sites"], name
        assert m["two_limb_grads_rel_l2"] < m["auto"]["grads_rel_l2"] < m["shift0"]["grads_rel_l2"], name
