"""Class-conditional NCSN++ and classifier-free guidance, host side: the config key, the one new parameter and where it
sits, the command-line arguments and the label-dropout mask (no GPU: nothing here launches a kernel)."""
import argparse

import pytest
import torch

import psld_amd
from psld_amd import cli
from psld_amd import config as C
from psld_amd.registry import get_module

PRESETS = ["c10_sota", "celeba64_sota", "afhqv2_128", "afhqv2_128_inpaint", "c10_ablation", "c10_vpsde", "yaml_default", "tiny",
           "tiny_vpsde"]


def _net(cfg):
    psld_amd.import_modules_into_registry()
    return get_module("score_fn", "ncsnpp")(cfg)


@pytest.mark.parametrize("name", PRESETS)
def test_presets_do_not_carry_the_key(name):
    cfg = getattr(C, name)()
    assert "label_classes" not in cfg.model.score_fn and "label_dropout" not in cfg.training
    assert "label_to_sample" not in cfg.evaluation and "cfg_scale" not in cfg.evaluation
    for clf in (C.clf_default(), C.clf_c10(), C.clf_afhqv2_128(), C.tiny_clf()):
        assert "label_classes" not in clf.model.clf_fn


def test_preset_network_keeps_its_state_dict():
    """A network without the key (and one with label_classes = 0) has the keys all_modules.<i>...., in module order, and
    nothing else; no parameter outside all_modules."""
    for cfg in (C.tiny(), C.tiny_vpsde()):
        net = _net(cfg)
        keys = list(net.state_dict().keys())
        assert all(k.startswith("all_modules.") for k in keys)
        idx = [int(k.split(".")[1]) for k in keys]
        assert idx == sorted(idx) and idx[0] == 0
        assert [k for k, _ in net.named_parameters()] == keys
        assert net.label_classes == 0 and net.label_emb is None
        cfg0 = getattr(C, "tiny" if cfg.model.sde.name == "psld" else "tiny_vpsde")()
        cfg0.model.score_fn.label_classes = 0
        assert list(_net(cfg0).state_dict().keys()) == keys


@pytest.mark.parametrize("name", ["tiny", "tiny_ablation", "c10_sota", "celeba64"])
def test_preset_network_has_the_recorded_keys_in_the_recorded_order(name):
    """Against the key / shape lists recorded with the reference's goldens (tests/golden/net_meta.json); and the conditional
    network has exactly those behind its one new key."""
    import json
    import os

    from tests.conftest import GOLDEN
    from tests.test_oracle_golden import _net_cfg
    with open(os.path.join(GOLDEN, "net_meta.json")) as fh:
        recorded = [(k, tuple(s)) for k, s in json.load(fh)[name]["keys"]]
    cfg = _net_cfg(name)
    assert [(k, tuple(v.shape)) for k, v in _net(cfg).state_dict().items()] == recorded
    cfg.model.score_fn.label_classes = 10
    got = [(k, tuple(v.shape)) for k, v in _net(cfg).state_dict().items()]
    assert got == [("label_emb", (11, 4 * cfg.model.score_fn.nf))] + recorded


@pytest.mark.parametrize("nf", [32, 128])
def test_conditional_network_has_one_more_parameter_at_the_front(nf):
    cfg = C.tiny(nf=nf)
    base = list(_net(cfg).state_dict().keys())
    cfg.model.score_fn.label_classes = 3
    net = _net(cfg)
    keys = list(net.state_dict().keys())
    assert keys == ["label_emb"] + base
    first = next(iter(net.parameters()))
    assert first is net.label_emb and isinstance(first, torch.nn.Parameter) and first.requires_grad
    assert tuple(first.shape) == (4, 4 * nf) and first.dtype == torch.float32
    assert float(first.detach().abs().max()) == 0.0
    # the flat layout puts it at offset 0 and moves nothing inside all_modules relative to each other
    offs, _ = net._layout()
    assert offs[id(net.label_emb)] == 0
    order = [offs[id(p)] for p in net.parameters()]
    assert order == sorted(order)
    import copy
    twin = copy.deepcopy(net)
    assert list(twin.state_dict().keys()) == keys and twin.label_classes == 3 and twin.label_emb is not net.label_emb


def test_classifier_and_unconditioned_embedding_refuse_the_key():
    psld_amd.import_modules_into_registry()
    clf = C.tiny_clf()
    clf.model.clf_fn.label_classes = 3
    with pytest.raises(ValueError, match="n_cls"):
        get_module("clf_fn", "ncsnpp_clf")(clf)
    get_module("clf_fn", "ncsnpp_clf")(C.tiny_clf())                   # without the key: as before
    cfg = C.tiny()
    cfg.model.score_fn.label_classes = 3
    cfg.model.score_fn.noise_cond = False
    with pytest.raises(ValueError, match="noise_cond"):
        _net(cfg)


def test_labels_for_a_network_without_classes_raise():
    """y (or drop) with K = 0 is a ValueError - raised by the argument check, before anything touches a device."""
    net = _net(C.tiny())
    x, t = torch.zeros(2, 6, 16, 16), torch.ones(2)
    y = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="label_classes"):
        net._labels(x, y)
    with pytest.raises(ValueError, match="label_classes"):
        net._labels(x, None, torch.zeros(2, dtype=torch.bool))
    assert net._labels(x, None) == (None, None)
    cfg = C.tiny()
    cfg.model.score_fn.label_classes = 3
    cnet = _net(cfg)
    lab, drop = cnet._labels(x, None)
    assert drop is None and lab.dtype == torch.int64 and lab.tolist() == [3, 3]          # None = the "no label" row K
    lab, drop = cnet._labels(x, y, torch.tensor([True, False]))
    assert lab.tolist() == [0, 0] and drop.dtype == torch.uint8 and drop.tolist() == [1, 0]
    for bad in (y.to(torch.int32), torch.zeros(3, dtype=torch.int64), [0, 0]):
        with pytest.raises(ValueError, match="int64"):
            cnet._labels(x, bad)


def test_cfg_score_fn_checks_its_arguments():
    from psld_amd.guidance import CFGScoreFn
    with pytest.raises(ValueError, match="label_classes"):
        CFGScoreFn(_net(C.tiny()), 0, 2.0)
    cfg = C.tiny()
    cfg.model.score_fn.label_classes = 3
    net = _net(cfg)
    with pytest.raises(ValueError, match="outside"):
        CFGScoreFn(net, 4, 2.0)
    with pytest.raises(ValueError, match="int64"):
        CFGScoreFn(net, torch.zeros(2, dtype=torch.int32), 2.0)
    fn = CFGScoreFn(net, 1, 2.0)
    assert not hasattr(fn, "vjp_input")
    net.train()
    assert fn.training and fn.eval() is fn and not fn.training and not net.training
    assert [id(p) for p in fn.parameters()] == [id(p) for p in net.parameters()]
    assert fn._labels(3, "cpu").tolist() == [1, 1, 1]
    assert CFGScoreFn(net, torch.tensor([2, 0, 1, 3]), 2.0)._labels(3, "cpu").tolist() == [2, 0, 1]


def test_wrapper_wraps_the_sampling_network_only_when_asked():
    from psld_amd.guidance import CFGScoreFn
    psld_amd.import_modules_into_registry()
    em = get_module("samplers", "em_sde")
    for k, label, wrapped in ((0, None, False), (3, None, False), (3, 2, True), (0, 2, False)):
        cfg = C.tiny()
        if k:
            cfg.model.score_fn.label_classes = k
        if label is not None:
            cfg.evaluation.label_to_sample = label
            cfg.evaluation.cfg_scale = 1.5
        net = _net(cfg)
        sde = get_module("sde", "psld")(cfg)
        for sample_from in ("target", "source"):
            cfg.evaluation.sample_from = sample_from
            ema = __import__("copy").deepcopy(net)
            wr = get_module("pl_modules", "sde_wrapper")(cfg, sde, net, ema_score_fn=ema, sampler_cls=em)
            fn = wr.sampler.score_fn
            chosen = ema if sample_from == "target" else net
            if wrapped:
                assert isinstance(fn, CFGScoreFn) and fn.net is chosen and fn.labels == 2 and fn.scale == 1.5
            else:
                assert fn is chosen
    cfg = C.tiny()
    cfg.model.score_fn.label_classes = 3
    cfg.evaluation.label_to_sample = 1
    net = _net(cfg)
    wr = get_module("pl_modules", "sde_wrapper")(cfg, get_module("sde", "psld")(cfg), net, ema_score_fn=net, sampler_cls=em)
    assert wr.sampler.score_fn.scale == 1.0                                 # evaluation.cfg_scale defaults to 1


# ---- command line ------------------------------------------------------------------------------------------------------
def _parse(argv):
    return cli.build_parser().parse_known_args(argv)


def test_parser_accepts_the_new_arguments():
    args, rest = _parse(["train", "--config", "tiny", "model.score_fn.label_classes=3", "--labels", "synthetic"])
    assert args.labels == "synthetic" and rest == ["model.score_fn.label_classes=3"]
    assert _parse(["train", "--config", "tiny"])[0].labels is None
    assert _parse(["train", "--labels", "y.npy"])[0].labels == "y.npy"
    assert _parse(["train_clf"])[0].labels == "synthetic"                   # train_clf keeps its default
    for cmd in ("sample", "inpaint"):
        args, _ = _parse([cmd, "--config", "tiny", "--label", "1", "--cfg-scale", "2.0"])
        assert args.label == 1 and args.cfg_scale == 2.0
        args, _ = _parse([cmd, "--config", "tiny"])
        assert args.label is None and args.cfg_scale is None
    for cmd in ("train", "train_clf", "cc_sample", "bpd"):                  # the other commands do not know the two arguments
        args, rest = _parse([cmd, "--cfg-scale", "2.0"])
        assert not hasattr(args, "cfg_scale") and not hasattr(args, "label") and rest == ["--cfg-scale", "2.0"]
    with pytest.raises(SystemExit):
        _parse(["sample", "--label", "one"])


def _cfg(k=0, **ev):
    cfg = C.tiny()
    if k:
        cfg.model.score_fn.label_classes = k
    for key, v in ev.items():
        cfg.evaluation[key] = v
    return cfg


def test_train_labels_are_required_with_classes_and_refused_without(tmp_path):
    ns = argparse.Namespace
    assert cli._train_labels(_cfg(), ns(labels=None), 8, "cpu") is None
    with pytest.raises(SystemExit, match="label_classes"):
        cli._train_labels(_cfg(), ns(labels="synthetic"), 8, "cpu")
    with pytest.raises(SystemExit, match="required"):
        cli._train_labels(_cfg(3), ns(labels=None), 8, "cpu")
    y = cli._train_labels(_cfg(3), ns(labels="synthetic"), 64, "cpu")
    assert y.dtype == torch.int64 and y.shape == (64,) and 0 <= int(y.min()) and int(y.max()) < 3
    assert torch.equal(y, cli._train_labels(_cfg(3), ns(labels="synthetic"), 64, "cpu"))        # the same on every rank
    import numpy as np
    path = str(tmp_path / "y.npy")
    np.save(path, np.array([0, 2, 1, 1], dtype=np.int32))
    assert cli._train_labels(_cfg(3), ns(labels=path), 4, "cpu").tolist() == [0, 2, 1, 1]
    np.save(path, np.array([0, 3, 1, 1]))                                   # 3 is the "no label" row: not a class
    with pytest.raises(SystemExit, match="outside"):
        cli._train_labels(_cfg(3), ns(labels=path), 4, "cpu")


def test_label_and_cfg_scale_are_spellings_of_the_config_keys():
    ns = argparse.Namespace
    cfg = cli.apply_label_args(_cfg(3), ns(label=1, cfg_scale=2.0))
    assert cfg.evaluation.label_to_sample == 1 and cfg.evaluation.cfg_scale == 2.0
    cfg = cli.apply_label_args(_cfg(3, label_to_sample=2), ns(label=None, cfg_scale=None))      # the keys alone work too
    assert cfg.evaluation.label_to_sample == 2 and "cfg_scale" not in cfg.evaluation
    cfg = cli.apply_label_args(_cfg(3, label_to_sample=2), ns(label=0, cfg_scale=None))         # the argument wins
    assert cfg.evaluation.label_to_sample == 0
    cfg = cli.apply_label_args(_cfg(), ns(label=None, cfg_scale=None))                          # nothing asked: untouched
    assert "label_to_sample" not in cfg.evaluation and "cfg_scale" not in cfg.evaluation
    with pytest.raises(SystemExit, match="label_classes"):
        cli.apply_label_args(_cfg(), ns(label=1, cfg_scale=None))
    with pytest.raises(SystemExit, match="outside"):
        cli.apply_label_args(_cfg(3), ns(label=3, cfg_scale=None))
    with pytest.raises(SystemExit, match="--label"):
        cli.apply_label_args(_cfg(3), ns(label=None, cfg_scale=2.0))


# ---- label dropout -----------------------------------------------------------------------------------------------------
def test_label_dropout_probability_follows_the_config():
    from psld_amd.losses import label_dropout_p
    cfg = C.tiny()
    assert label_dropout_p(cfg) == 0.0
    cfg.training.label_dropout = 0.5                                        # ignored without classes
    assert label_dropout_p(cfg) == 0.0
    cfg = C.tiny()
    cfg.model.score_fn.label_classes = 3
    assert label_dropout_p(cfg) == 0.1
    cfg.training.label_dropout = 0.25
    assert label_dropout_p(cfg) == 0.25
    cfg.training.label_dropout = 0
    assert label_dropout_p(cfg) == 0.0
    psld_amd.import_modules_into_registry()
    sde = get_module("sde", "psld")(cfg)
    assert get_module("losses", "psld_score_loss")(cfg, sde).label_dropout == 0.0
    assert get_module("losses", "psld_score_loss")(C.tiny(), sde).label_dropout == 0.0


def test_label_drop_mask_is_one_uniform_draw():
    from psld_amd.losses import label_drop_mask
    g = torch.Generator().manual_seed(5)
    state = g.get_state()
    assert label_drop_mask(16, 0.0, "cpu", g) is None and label_drop_mask(16, -1.0, "cpu", g) is None
    assert torch.equal(g.get_state(), state)                                # p <= 0: no draw at all
    m = label_drop_mask(16, 0.3, "cpu", g)
    u = torch.rand(16, generator=torch.Generator().manual_seed(5))
    assert m.dtype == torch.bool and torch.equal(m, u < 0.3) and 0 < int(m.sum()) < 16
    g2 = torch.Generator().manual_seed(5)
    torch.rand(16, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())                       # exactly one rand(B)
    assert bool(label_drop_mask(16, 1.0, "cpu", g).all())                   # u in [0, 1): p = 1 drops every label
