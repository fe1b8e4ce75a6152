"""AFHQv2-128 without a GPU: the 3x3 limb kernels' shape rules take 128-wide maps (and keep today's answers elsewhere), the
presets equal the reference's afhqv2128_psld.yaml + train script (tests/golden/afhq_meta.json, tools/gen_golden_afhq.py),
the network's state dict is the reference's, and the command line accepts the preset."""
import json
import os

import pytest

from psld_amd import _lib
from psld_amd import config as C
from tests.conftest import GOLDEN


def _meta():
    with open(os.path.join(GOLDEN, "afhq_meta.json")) as fh:
        return json.load(fh)


def test_limb_kernel_shape_rules_take_128_wide_maps():
    lib = _lib.load()
    assert lib.psld_conv3x3_wino_supported(128, 0, 8, 128, 128, 128) == 1
    assert lib.psld_conv3x3_wino_supported(128, 128, 1, 128, 128, 128) == 1
    assert lib.psld_conv3x3_wino_supported(256, 0, 2, 128, 128, 128) == 1
    assert lib.psld_conv3x3_wino_gn_supported(128, 0, 8, 128, 128, 128) == 1
    assert lib.psld_conv3x3_split_supported(128, 0, 8, 128, 128, 128) == 1
    assert lib.psld_conv3x3_split_supported(128, 128, 1, 128, 128, 128) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(128, 128, 0, 8, 128, 128) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(128, 128, 128, 1, 128, 128) == 1
    assert lib.psld_conv3x3_wgrad_wino_nsplit(128, 128, 8, 128, 128) >= 1
    assert lib.psld_conv3x3_wgrad_split_supported(128, 128, 8, 128, 128) == 1
    # the 128-wide geometry's own limits: Winograd 4 x 32 blocks need h % 4, the direct 2 x 64 blocks h % 2
    assert lib.psld_conv3x3_wino_supported(128, 0, 1, 126, 128, 128) == 0
    assert lib.psld_conv3x3_split_supported(128, 0, 1, 127, 128, 128) == 0
    assert lib.psld_conv3x3_split_supported(128, 0, 1, 126, 128, 128) == 1
    # wider maps stay out of scope
    for fn in (lib.psld_conv3x3_wino_supported, lib.psld_conv3x3_split_supported):
        assert fn(128, 0, 1, 256, 256, 128) == 0
    assert lib.psld_conv3x3_wgrad_wino_supported(128, 128, 0, 1, 256, 256) == 0
    assert lib.psld_conv3x3_wgrad_split_supported(128, 128, 1, 256, 256) == 0


@pytest.mark.parametrize("args,want", [
    ((128, 0, 16, 32, 32, 256), 1), ((256, 256, 128, 8, 8, 256), 1), ((64, 32, 2, 16, 16, 128), 1),
    ((32, 0, 1, 64, 64, 128), 1), ((32, 0, 2, 4, 8, 128), 1),
    ((6, 0, 2, 32, 32, 128), 0), ((128, 0, 2, 32, 32, 6), 0), ((64, 0, 2, 12, 12, 128), 0), ((128, 0, 2, 32, 32, 96), 0),
])
def test_limb_kernel_shape_rules_keep_todays_answers(args, want):
    lib = _lib.load()
    assert lib.psld_conv3x3_split_supported(*args) == want
    c1, c2, b, h, w, co = args
    assert lib.psld_conv3x3_wino_supported(*args) == (want if (h * w >= 128 or 128 % (h * w) == 0) else 0)


def test_weight_gradient_shape_rules_keep_todays_answers():
    lib = _lib.load()
    assert lib.psld_conv3x3_wgrad_split_supported(96, 64, 2, 8, 8) == 0
    assert lib.psld_conv3x3_wgrad_split_supported(128, 64, 2, 64, 64) == 1
    assert lib.psld_conv3x3_wgrad_split_supported(256, 256, 16, 32, 32) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(256, 256, 0, 16, 32, 32) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(128, 128, 0, 2, 64, 64) == 1
    assert lib.psld_conv3x3_wgrad_wino_supported(128, 64, 0, 2, 32, 32) == 0
    assert lib.psld_conv3x3_wgrad_wino_supported(128, 128, 0, 2, 32, 16) == 0


def _same(a, b):
    if isinstance(a, (int, float)) and isinstance(b, (int, float)) and not isinstance(a, bool):
        return float(a) == float(b)
    if isinstance(a, str) and isinstance(b, (int, float)):
        return float(a) == float(b)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_afhqv2_128_preset_equals_the_reference_configuration():
    m = _meta()["diffusion"]
    c = C.afhqv2_128()
    for node, want in (("data", c.data), ("score_fn", c.model.score_fn), ("sde", c.model.sde),
                       ("optimizer", c.training.optimizer), ("loss", c.training.loss), ("training", c.training),
                       ("evaluation", c.evaluation)):
        for k, v in m[node].items():
            assert _same(v, want[k]), (node, k, v, want[k])
    assert c.training.batch_size == 8 and c.data.image_size == 128 and c.model.score_fn.ch_mult == [1, 2, 2, 2, 3]


def test_clf_afhqv2_128_preset_equals_the_reference_configuration():
    m = _meta()["clf"]
    c = C.clf_afhqv2_128()
    for node, want in (("data", c.data), ("clf_fn", c.model.clf_fn), ("optimizer", c.training.optimizer),
                       ("training", c.training)):
        for k, v in m[node].items():
            assert _same(v, want[k]), (node, k, v, want[k])


def test_afhqv2_128_state_dict_census_is_the_references():
    import psld_amd
    psld_amd.import_modules_into_registry()
    from psld_amd.registry import get_module
    m = _meta()
    net = get_module("score_fn", "ncsnpp")(C.afhqv2_128())
    ks = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert len(ks) == m["n_keys"] == 450
    assert ks == m["keys"]
    assert sum(p.numel() for p in net.parameters()) == m["n_params"] == 65816582


def test_cli_accepts_the_afhqv2_128_presets():
    from psld_amd import cli
    args, rest = cli.build_parser().parse_known_args(["train", "--config", "afhqv2_128", "dataset.diffusion.training.batch_size=4"])
    assert args.config == "afhqv2_128" and rest == ["dataset.diffusion.training.batch_size=4"]
    cfg = cli.parse_overrides(getattr(C, args.config)(), rest)
    assert cfg.training.batch_size == 4 and cfg.data.image_size == 128
    args, _ = cli.build_parser().parse_known_args(["cc_sample", "--config", "afhqv2_128", "--clf-config", "clf_afhqv2_128"])
    assert getattr(C, args.clf_config)().model.clf_fn.n_cls == 3
