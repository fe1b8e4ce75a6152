"""CPU tests of psld_amd.weight_cache: staleness, batched family refreshes, in-place buffers, the graph-replay refresh,
driven by fake builders / launchers that record their calls on CPU tensors."""
import copy

import torch

from psld_amd import config as C
from psld_amd.weight_cache import Entry, WeightCache


class Recorder:
    def __init__(self):
        self.calls = []

    def launcher(self, name):
        def launch(table, rows, total):
            self.calls.append((name, rows, total, table.data_ptr()))
        return launch

    def entry(self, family=None, graph=False, filled=False):
        """make(owner, tag) of an entry whose buffer is 2 * owner (``filled``: made allocated, filled by the family)."""
        def make(owner, tag):
            def build(prev):
                self.calls.append(("build", tag))
                out = prev if prev is not None else torch.empty_like(owner)
                return out.copy_(owner * 2)

            def rows(out):
                return [([owner.data_ptr(), out.data_ptr()], owner.numel())]
            return Entry(owner, out=torch.empty_like(owner) if filled else None, build=None if filled else build,
                         family=family, rows=rows, graph=graph)
        return make


def _cache(rec):
    return WeightCache({"limb": (rec.launcher("limb"), 2), "copy": (rec.launcher("copy"), 1)})


def test_an_entry_goes_stale_on_write_invalidate_and_moved_storage():
    rec = Recorder()
    wc = _cache(rec)
    p = torch.nn.Parameter(torch.ones(4))
    make = rec.entry()
    out = wc.get(p, "a", make, "a")
    assert rec.calls == [("build", "a")] and torch.equal(out, 2 * p.detach())
    ptr = out.data_ptr()
    assert wc.get(p, "a", make, "a") is out and len(rec.calls) == 1             # fresh: no work
    with torch.no_grad():
        p.add_(1.0)                                                            # in-place write: _version moves
    assert torch.equal(wc.get(p, "a", make, "a"), torch.full((4,), 4.0)) and len(rec.calls) == 2
    wc.invalidate()                                                            # a raw-pointer write (optimiser / EMA)
    wc.get(p, "a", make, "a")
    assert len(rec.calls) == 3
    p.data = p.data.clone()                                                    # storage moved
    wc.get(p, "a", make, "a")
    assert len(rec.calls) == 4 and wc.get(p, "a", make, "a").data_ptr() == ptr  # refreshed in place every time
    assert len(rec.calls) == 4


def test_one_stale_access_refreshes_a_family_with_one_launch():
    rec = Recorder()
    wc = _cache(rec)
    ps = [torch.nn.Parameter(torch.randn(8)) for _ in range(3)]
    make = rec.entry(family="limb")
    outs = [wc.get(p, "f", make, "f%d" % i) for i, p in enumerate(ps)]
    assert rec.calls == [("build", "f0"), ("build", "f1"), ("build", "f2")]     # first use: built alone
    ptrs = [o.data_ptr() for o in outs]
    rec.calls.clear()
    wc.invalidate()
    wc.get(ps[1], "f", make)
    assert len(rec.calls) == 1 and rec.calls[0][:3] == ("limb", 3, 24)          # ONE launch covering all three
    table = rec.calls[0][3]
    for p in ps:
        wc.get(p, "f", make)
    assert len(rec.calls) == 1                                                 # the others are fresh now
    assert [wc.get(p, "f", make).data_ptr() for p in ps] == ptrs
    wc.invalidate()
    wc.get(ps[0], "f", make)
    assert rec.calls[1] == ("limb", 3, 24, table)                              # same entries and pointers: same table
    # a family below its minimum falls back to rebuilding the entry alone
    rec2 = Recorder()
    wc2 = _cache(rec2)
    q = torch.nn.Parameter(torch.randn(8))
    o = wc2.get(q, "f", rec2.entry(family="limb"), "solo")
    wc2.invalidate()
    assert wc2.get(q, "f", None).data_ptr() == o.data_ptr()
    assert rec2.calls == [("build", "solo"), ("build", "solo")]


def test_a_gathered_copy_is_refreshed_by_its_family_from_first_use():
    rec = Recorder()
    wc = _cache(rec)
    p, q = torch.nn.Parameter(torch.randn(4)), torch.nn.Parameter(torch.randn(8))
    make = rec.entry(family="copy", filled=True)
    e = wc.entry(p, "bias", make, "b")
    assert rec.calls == [] and e.stamp is None                                 # allocated, not yet filled
    out = wc.fresh(e)
    assert [c[:3] for c in rec.calls] == [("copy", 1, 4)] and out is e.out
    wc.get(q, "bias", make, "b")
    assert [c[:3] for c in rec.calls] == [("copy", 1, 4), ("copy", 2, 12)]     # a new member: all of them


def test_the_graph_refresh_touches_exactly_the_replayed_entries():
    rec = Recorder()
    wc = _cache(rec)
    a, b, c, d = (torch.nn.Parameter(torch.randn(4)) for _ in range(4))
    wc.get(a, "t", rec.entry(graph=True), "a")
    wc.get(b, "t", rec.entry(graph=False), "b")
    wc.get(c, "t", rec.entry(family="limb", graph=True), "c")
    wc.get(d, "t", rec.entry(family="limb", graph=False), "d")
    rec.calls.clear()
    wc.invalidate()
    wc.refresh(forward_only=True)
    assert [c[:3] for c in rec.calls] == [("build", "a"), ("limb", 2, 8)]
    stale = [p for p in (a, b, c, d) if wc.entries[(id(p), "t")].stamp != wc.stamp(p)]
    assert stale == [b]                                                        # the batch still covers its whole family
    rec.calls.clear()
    wc.refresh(forward_only=True)
    assert rec.calls == []
    wc.refresh(forward_only=False)
    assert rec.calls == [("build", "b")]


def test_a_deep_copied_network_starts_with_an_empty_cache():
    from psld_amd.score_fn import NCSNpp
    net = NCSNpp(C.tiny(image_size=8, nf=16, ch_mult=(1,), num_res_blocks=1, attn_resolutions=(8,)))
    net.flatten_parameters()
    rec = Recorder()
    w = net.all_modules[-1].weight
    buf = net._wcache.get(w, "t", rec.entry(graph=True), "t")
    ema = copy.deepcopy(net)
    assert ema._wcache is not net._wcache and not ema._wcache.entries and ema._wcache.epoch == 0
    assert (id(w), "t") in net._wcache.entries
    assert ema._flat is None and ema._graphs == {} and ema._tables is not net._tables
    assert ema.use_graphs == net.use_graphs and ema.defer_param_grads == net.defer_param_grads
    ptrs = {p.data_ptr() for p in net.parameters()} | {buf.data_ptr()}
    assert not ptrs & {p.data_ptr() for p in ema.parameters()}
    for p, q in zip(net.parameters(), ema.parameters()):
        assert torch.equal(p, q)
