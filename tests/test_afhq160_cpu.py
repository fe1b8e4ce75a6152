"""The AFHQv2-128 inpainting network (nf = 160) without a GPU: the Winograd limb kernels' shape rules take channel widths
that are multiples of 32 from 128 up (and keep every other answer), the ``afhqv2_128_inpaint`` preset equals the reference's
afhqv2128_psld.yaml + sample_inpaint_psld.sh (tests/golden/afhq160_meta.json, tools/gen_golden_afhq160.py), the network's
state dict is the reference's, and the command line accepts the preset."""
import json
import os

import pytest

from psld_amd import _lib
from psld_amd import config as C
from tests.conftest import GOLDEN
from tests.test_afhq_cpu import _same


def _meta():
    with open(os.path.join(GOLDEN, "afhq160_meta.json")) as fh:
        return json.load(fh)


def test_winograd_shape_rules_take_the_nf160_widths():
    lib = _lib.load()
    assert lib.psld_conv3x3_wino_supported(160, 0, 1, 128, 128, 160) == 1
    assert lib.psld_conv3x3_wino_supported(320, 160, 2, 64, 64, 320) == 1
    assert lib.psld_conv3x3_wino_supported(480, 480, 2, 8, 8, 480) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(160, 160, 0, 8, 128, 128) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(480, 320, 0, 2, 16, 16) == 1
    # the GroupNorm-fused staging keeps whole 128-channel tiles
    assert lib.psld_conv3x3_wino_gn_supported(160, 0, 1, 128, 128, 160) == 0
    assert lib.psld_conv3x3_wino_gn_supported(320, 160, 2, 64, 64, 320) == 0
    assert lib.psld_conv3x3_wino_gn_supported(480, 480, 2, 8, 8, 480) == 0
    # K splits and workspace of the tail shapes
    assert lib.psld_conv3x3_wgrad_wino_nsplit(160, 160, 8, 128, 128) >= 1
    assert lib.psld_conv3x3_wgrad_wino_nsplit(480, 960, 16, 8, 8) >= 1
    assert lib.psld_conv3x3_wino_frag_bytes(160, 480) == 160 * 480 * 96 + 16384


def _old_wino(c1, c2, cout):
    return cout % 128 == 0


def _old_wgrad(cout, cin, cin2):
    return cout % 128 == 0 and cin % 128 == 0 and cin2 % 128 == 0


WIDTHS = range(32, 513, 32)


@pytest.mark.parametrize("b,s", [(2, 8), (4, 16), (1, 64), (1, 128)])
def test_forward_rule_sweep_changes_only_tail_widths(b, s):
    """cout and cin over {32, 64, ..., 512}: where the old rule (cout % 128) held the answer is unchanged, below 128 it is
    unchanged, and only widths that are multiples of 32 from 128 up change - from 0 to 1."""
    lib = _lib.load()
    full = lib.psld_conv3x3_wino_supported(128, 0, b, s, s, 128)
    assert full == 1
    for cin in WIDTHS:
        for cout in WIDTHS:
            got = lib.psld_conv3x3_wino_supported(cin, 0, b, s, s, cout)
            if _old_wino(cin, 0, cout) or cout < 128:
                assert got == (full if cout % 128 == 0 else 0), (cin, cout)
            else:
                assert got == 1, (cin, cout)
            # the fused GroupNorm staging keeps today's rule
            assert lib.psld_conv3x3_wino_gn_supported(cin, 0, b, s, s, cout) == \
                (lib.psld_conv3x3_wino_gn_supported(cin, 0, b, s, s, 128) if cout % 128 == 0 else 0), (cin, cout)


@pytest.mark.parametrize("b,s", [(4, 8), (4, 16), (1, 64), (1, 128)])
def test_weight_gradient_rule_sweep_changes_only_tail_widths(b, s):
    """The same sweep for the Winograd-domain weight gradient over cout and cin (one source)."""
    lib = _lib.load()
    full = lib.psld_conv3x3_wgrad_wino_supported(128, 128, 0, b, s, s)
    assert full == 1
    for cin in WIDTHS:
        for cout in WIDTHS:
            got = lib.psld_conv3x3_wgrad_wino_supported(cout, cin, 0, b, s, s)
            if _old_wgrad(cout, cin, 0) or cout < 128 or cin < 128:
                assert got == (full if _old_wgrad(cout, cin, 0) else 0), (cout, cin)
            else:
                assert got == 1, (cout, cin)


def test_weight_gradient_two_sources():
    """A second source starts on a 128-channel c_in tile; it may end in a tail."""
    lib = _lib.load()
    assert lib.psld_conv3x3_wgrad_wino_supported(160, 128, 160, 1, 64, 64) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(128, 128, 128, 1, 128, 128) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(160, 160, 160, 1, 64, 64) == 0      # a c_in tile would straddle the sources
    assert lib.psld_conv3x3_wgrad_wino_supported(160, 128, 96, 1, 64, 64) == 0
    assert lib.psld_conv3x3_wgrad_wino_supported(160, 128, 64, 1, 64, 64) == 0


def test_direct_kernel_rules_unchanged():
    """The direct limb kernels keep their rules (the Winograd forms take every 3x3 layer of the nf = 160 network)."""
    lib = _lib.load()
    assert lib.psld_conv3x3_split_supported(160, 0, 1, 128, 128, 160) == 0
    assert lib.psld_conv3x3_split_supported(128, 0, 2, 32, 32, 96) == 0
    assert lib.psld_conv3x3_wgrad_split_supported(160, 160, 8, 128, 128) == 0
    assert lib.psld_conv3x3_wgrad_split_supported(96, 64, 2, 8, 8) == 0


def test_afhqv2_128_inpaint_preset_equals_the_reference_configuration():
    m = _meta()["diffusion"]
    c = C.afhqv2_128_inpaint()
    for node, want in (("data", c.data), ("score_fn", c.model.score_fn), ("sde", c.model.sde)):
        for k, v in m[node].items():
            assert _same(v, want[k]), (node, k, v, want[k])
    for k, v in m["evaluation"].items():
        if k == "sampler":
            assert c.evaluation.sampler.name == v["name"] == "ip_em_sde"
        else:
            assert _same(v, c.evaluation[k]), (k, v, c.evaluation[k])
    assert c.model.score_fn.nf == 160 and c.model.score_fn.ch_mult == [1, 2, 2, 3, 3] and c.model.sde.gamma == 0


def test_afhqv2_128_inpaint_state_dict_census_is_the_references():
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    m = _meta()
    net = get_module("score_fn", "ncsnpp")(C.afhqv2_128_inpaint())
    ks = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert len(ks) == m["n_keys"] == 480
    assert ks == m["keys"]
    assert sum(p.numel() for p in net.parameters()) == m["n_params"] == 128449443


def test_cli_accepts_the_afhqv2_128_inpaint_preset():
    from psld_amd import cli
    args, rest = cli.build_parser().parse_known_args(["inpaint", "--config", "afhqv2_128_inpaint", "--mask", "synthetic",
                                                      "evaluation.n_discrete_steps=3"])
    assert args.config == "afhqv2_128_inpaint" and args.mask == "synthetic" and rest == ["evaluation.n_discrete_steps=3"]
    cfg = cli.parse_overrides(getattr(C, args.config)(), rest)
    assert cfg.evaluation.n_discrete_steps == 3 and cfg.model.score_fn.nf == 160 and cfg.data.image_size == 128
