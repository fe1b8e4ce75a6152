"""Bookkeeping of the guard-band harness (tests/guard.py) on a CPU tensor: offsets, exact sizes, no reuse before check(),
the exhaustion error, and both failure modes of run_guarded with plain torch standing in for a kernel."""
import pytest
import torch

from tests import guard as G

BAND = 4096          # small bands: the bookkeeping does not depend on their width


def _pool(nbytes=1 << 20):
    return G.GuardPool("cpu", nbytes, band=BAND)


def test_views_have_exact_sizes_aligned_starts_and_bands_on_both_sides():
    pool = _pool()
    a = pool.take((3, 5, 7), torch.float32, "a")
    b = pool.take_bytes(1, "b")
    c = pool.take((11,), torch.float64, "c")
    z = pool.take_bytes(0, "empty")
    assert a.shape == (3, 5, 7) and a.dtype == torch.float32 and b.numel() == 1 and c.numel() == 11 and z.numel() == 0
    base = pool.buf.data_ptr()
    prev_end = 0
    for (name, start, end), t in zip(pool.regions, (a, b, c, z)):
        if t.numel():          # (torch reports a null data_ptr for an empty view)
            assert t.data_ptr() == base + start and t.data_ptr() % G.ALIGN == 0, name
        assert (base + start) % G.ALIGN == 0, name
        assert end - start == t.numel() * t.element_size(), name          # exactly the bytes asked for, no rounding
        assert start - prev_end >= BAND, name                               # a full band before ...
        prev_end = end
    assert pool.buf.numel() - prev_end >= BAND                              # ... and after the last one
    # the trailing band starts at the first byte after the request
    assert pool.buf[pool.regions[1][2]] == G.PATTERN and pool.buf[pool.regions[1][1] - 1] == G.PATTERN
    assert bool((pool.buf[:pool.regions[0][1]] == G.PATTERN).all())
    pool.check()


def test_nothing_is_handed_out_twice_and_release_needs_a_check():
    pool = _pool()
    spans = []
    for i in range(20):
        pool.take_bytes(100 + i, f"t{i}")
        spans.append(pool.regions[-1][1:])
    for (s0, e0), (s1, e1) in zip(spans, spans[1:]):
        assert s1 >= e0 + BAND
    with pytest.raises(AssertionError, match="before check"):
        pool.release()
    pool.check()
    pool.release()
    assert pool.regions == [] and bool((pool.buf == G.PATTERN).all())
    first = pool.take_bytes(100, "again")
    assert first.data_ptr() == pool.buf.data_ptr() + spans[0][0]            # addresses repeat after a release


def test_a_full_pool_fails_loudly_and_does_not_wrap():
    pool = _pool(64 * 1024)
    pool.take_bytes(20000, "big")
    with pytest.raises(G.GuardPoolFull, match="never wraps"):
        pool.take_bytes(40000, "too much")
    assert len(pool.regions) == 1
    pool.check()


def test_check_names_the_buffer_and_the_first_offset():
    pool = _pool()
    pool.take((4,), torch.float32, "left")
    t = pool.take((10,), torch.float32, "victim")
    pool.take((4,), torch.float32, "right")
    start, end = pool.regions[1][1:]
    pool.buf[end + 8] = 0                                                   # 9th byte after the view
    with pytest.raises(G.GuardViolation, match=r"8 bytes past the end of 'victim'"):
        pool.check()
    pool.buf[end + 8] = G.PATTERN
    pool.buf[start - 1] = 1                                                 # the byte before it
    with pytest.raises(G.GuardViolation, match=r"1 bytes before the start of 'victim'"):
        pool.check()
    pool.buf[start - 1] = G.PATTERN
    t.fill_(0.0)                                                            # writing the view itself is fine
    pool.check()


class _FakeOps:
    """run_guarded needs an object with ``workspace`` and ``torch`` attributes to patch; no kernel runs here."""
    torch = torch

    @staticmethod
    def workspace(nbytes, device):
        return torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)


def _guard():
    ops = _FakeOps()
    g = G.Guard(ops, _pool(4 << 20))
    ops.workspace, ops.torch = g.workspace, g.torch
    return g, ops


def test_run_guarded_passes_a_clean_op_and_catches_both_failure_modes():
    g, ops = _guard()
    x = torch.arange(12, dtype=torch.float32).view(3, 4)
    wide = torch.zeros(3, 6)

    def clean(x, y, wide):
        y.copy_(x * 2)
        wide[:, 1:5] = x
        ws = ops.workspace(48, x.device)
        assert (ws.numel() == 48) == g.active                             # guarded: exactly the bytes asked for
        return ops.torch.empty((3,), dtype=torch.float32, device=x.device).copy_(x.sum(1))

    plain, ret = G.run_guarded(g, clean, dict(x=x, y=torch.full((3, 4), float("nan")), wide=wide), {"y": None, "wide": (1, 5)})
    assert torch.equal(plain["y"], x * 2) and torch.equal(ret, x.sum(1))

    def writes_past(x, y):
        y.copy_(x * 2)
        if g.active:       # one element past the guarded view, through a wider view of the pool
            off = y.data_ptr() - g.pool.buf.data_ptr()
            g.pool.buf[off + y.numel() * 4:off + y.numel() * 4 + 4] = 0
    with pytest.raises(G.GuardViolation, match="past the end of 'y'"):
        G.run_guarded(g, writes_past, dict(x=x, y=torch.zeros(3, 4)), ["y"])

    def reads_past(x, y):
        if g.active:
            off = x.data_ptr() - g.pool.buf.data_ptr()
            src = g.pool.buf[off:off + (x.numel() + 1) * 4].view(torch.float32)
        else:
            src = torch.cat([x.reshape(-1), torch.zeros(1)])
        y.fill_(float(src.sum()))
    with pytest.raises(G.GuardViolation, match=r"\(b\) output 'y' differs"):
        G.run_guarded(g, reads_past, dict(x=x, y=torch.zeros(3, 4)), ["y"])

    def writes_gap(x, wide):
        wide[:, 1:5] = x
        if g.active:
            wide[2, 5] = 0.0
    with pytest.raises(AssertionError, match="gap columns of 'wide'"):
        G.run_guarded(g, writes_gap, dict(x=x, wide=wide), {"wide": (1, 5)})

    def clobbers_input(x, y):
        y.copy_(x)
        if g.active:
            x[0, 0] = -1.0
    with pytest.raises(AssertionError, match=r"\(c\) input 'x' changed"):
        G.run_guarded(g, clobbers_input, dict(x=x, y=torch.zeros(3, 4)), ["y"])


def test_guarded_arena_keeps_the_parents_bookkeeping():
    from psld_amd import ops
    Arena = G.make_guarded_arena(ops)
    a = Arena("cpu", 1 << 20)
    s1, s2 = a.alloc(100), a.floats(3, 5)
    assert s1.numel() == 100 and s2.shape == (3, 5) and s1.data_ptr() % G.ALIGN == 0 and s2.data_ptr() % G.ALIGN == 0
    assert s2.data_ptr() - (s1.data_ptr() + 100) >= G.ARENA_BAND
    p1, p2 = s1.data_ptr(), s2.data_ptr()
    s1.fill_(0)
    s2.fill_(1.0)
    a.reset()
    assert a.off == 0 and a.high > 0 and a.retired == []
    assert (a.alloc(100).data_ptr(), a.floats(3, 5).data_ptr()) == (p1, p2)        # addresses repeat from step to step
    assert a.violations() == 0
    t = a.alloc(64)
    off = t.data_ptr() - a.buf.data_ptr()
    a.buf[off + 64] = 0                                                            # first byte past the slice
    a.buf[off - 1] = 0
    assert a.violations() == 2
    big = a.alloc(2 << 20)                                                         # outgrows the buffer: the parent's growth
    assert big.numel() == 2 << 20 and len(a.retired) == 1 and bool((a.buf[:G.ARENA_BAND] == G.PATTERN).all())
    a.reset()
    assert a.retired == [] and a.violations() == 2
