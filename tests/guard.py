"""Guard bands: a software bounds checker for the HIP kernels (a helper module of tests/test_bounds_gpu.py).

The suite compares VALUES; this module checks WHERE a kernel reads and writes.  Every buffer a guarded call sees has
exactly the documented number of bytes, starts on a 256-byte boundary and lies between two bands of a fixed byte pattern
inside one live allocation the test owns:

* a write outside the buffer changes a band (``GuardPool.check`` names the buffer and the first offending offset);
* a read outside the buffer that reaches a result reads 0xFF bytes - NaN in fp32, fp64 and bf16 - and the result differs
  from the same call on ordinary buffers (``run_guarded`` compares bit for bit).

What it cannot see: a read outside a buffer that never reaches a result, and an access farther from the buffer than the
band is wide (1 MiB around pool buffers, 64 KiB around arena slices).
"""
from __future__ import annotations

import torch

PATTERN = 0xFF            # every byte of a band: NaN as fp32, fp64 and bf16
ALIGN = 256               # buffer starts (what ops.Arena and the caching allocator hand the product as well)
BAND = 1 << 20            # bytes of pattern on each side of a pool buffer
ARENA_BAND = 64 << 10     # ... of an arena slice


class GuardViolation(AssertionError):
    pass


class GuardPoolFull(RuntimeError):
    pass


def _nbytes(shape, dtype) -> int:
    n = torch.empty((), dtype=dtype).element_size()
    for d in shape:
        n *= int(d)
    return n


class GuardPool:
    """One uint8 allocation handing out exact-size views separated by pattern bands.  Neighbouring views share the band
    between them (the trailing band of one is the leading band of the next, at least ``band`` bytes).  Nothing is handed
    out twice before ``check()``; ``release()`` (only after a check) makes the pool empty again."""

    def __init__(self, device, nbytes: int, band: int = BAND):
        self.band = int(band)
        self.buf = torch.full((int(nbytes),), PATTERN, dtype=torch.uint8, device=device)
        self.base = (-self.buf.data_ptr()) % ALIGN      # offset of the first aligned byte
        self.regions = []                               # (name, start, end) in bytes of buf
        self.end = self.base                            # first byte after the last view
        self.peak = 0
        self._checked = True

    # -- bookkeeping ------------------------------------------------------------------------------------------------
    def _next_start(self) -> int:
        start = self.end + self.band
        return start + (-(start - self.base)) % ALIGN

    def take_bytes(self, n: int, name: str = "") -> torch.Tensor:
        n = int(n)
        assert n >= 0
        start = self._next_start()
        if start + n + self.band > self.buf.numel():
            raise GuardPoolFull(f"guard pool of {self.buf.numel()} bytes is full: {len(self.regions)} buffers to byte "
                                f"{self.end}, asked for {n} more ({name or 'unnamed'}); the pool never wraps")
        self.regions.append((name or f"buffer{len(self.regions)}", start, start + n))
        self.end = start + n
        self.peak = max(self.peak, self.end + self.band)
        self._checked = False
        return self.buf[start:start + n]

    def take(self, shape, dtype, name: str = "") -> torch.Tensor:
        shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        return self.take_bytes(_nbytes(shape, dtype), name).view(dtype).view(shape)

    def take_like(self, t: torch.Tensor, name: str = "") -> torch.Tensor:
        """A guarded copy of a contiguous tensor (python attributes such as ``fine_width`` travel along)."""
        assert t.is_contiguous()
        g = self.take(t.shape, t.dtype, name)
        g.copy_(t)
        for k, v in getattr(t, "__dict__", {}).items():
            setattr(g, k, v)
        return g

    def gaps(self):
        """(name of the buffer before the gap or '', name of the buffer after it or '', start, end) of every band."""
        out, prev_end, prev = [], 0, ""
        for name, start, end in self.regions:
            out.append((prev, name, prev_end, start))
            prev_end, prev = end, name
        out.append((prev, "", prev_end, min(self.buf.numel(), prev_end + self.band + ALIGN) if self.regions else self.buf.numel()))
        return out

    # -- the check ------------------------------------------------------------------------------------------------------
    def check(self):
        """Every band byte is still the pattern, else GuardViolation naming the buffer and the first offending offset."""
        gaps = self.gaps()
        bad = torch.stack([torch.count_nonzero(self.buf[a:b] != PATTERN) for _, _, a, b in gaps]).cpu()
        self._checked = True
        for (before, after, a, b), n in zip(gaps, bad.tolist()):
            if n == 0:
                continue
            first = a + int(torch.nonzero(self.buf[a:b] != PATTERN)[0, 0])
            last = a + int(torch.nonzero(self.buf[a:b] != PATTERN)[-1, 0])
            msgs = []
            if before:
                end = next(e for nm, _, e in self.regions if nm == before and e == a)
                msgs.append(f"{first - end} bytes past the end of '{before}'")
            if after:
                msgs.append(f"{b - last} bytes before the start of '{after}'")
            raise GuardViolation(f"{n} guard-band bytes changed: first at " + ", last at ".join(msgs) +
                                 f" (pool offsets {first} .. {last})")

    def release(self):
        """Forget every buffer and restore the pattern.  Only after check(): nothing is reused unchecked."""
        assert self._checked, "GuardPool.release() before check(): a region would be reused unchecked"
        hi = min(self.buf.numel(), self.end + self.band + ALIGN)
        self.buf[:hi].fill_(PATTERN)
        self.regions, self.end = [], self.base


# ---------------------------------------------------------------------------------------------------------------------
# redirecting the product's own allocations
# ---------------------------------------------------------------------------------------------------------------------
class _TorchProxy:
    """Stands in for the ``torch`` module inside psld_amd.ops: while the guard is active, ``empty`` / ``empty_like`` of
    device tensors (the outputs the wrappers allocate themselves) come from the pool; everything else is torch."""

    def __init__(self, guard):
        self._guard = guard

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=None, device=None, **kw):
        g = self._guard
        if not g.active or device is None or torch.device(device).type != g.pool.buf.device.type:
            return torch.empty(*shape, dtype=dtype, device=device, **kw)
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        return g.pool.take(shape, dtype or torch.float32, "ops.empty")

    def empty_like(self, t, **kw):
        g = self._guard
        if not g.active or kw or t.device.type != g.pool.buf.device.type:
            return torch.empty_like(t, **kw)
        return g.pool.take(t.shape, t.dtype, "ops.empty_like")


class Guard:
    """The pool plus the patches of psld_amd.ops the new tests install through pytest's monkeypatch: ``workspace`` (exactly
    ``nbytes`` bytes, no 1 MiB floor, fresh on every call), the allocation of wrapper-owned outputs (``outputs=True``) and the
    slot buffer of the team kernels (``gn_team_sync``: zeroed, exactly psld_gn_bwd_team_sync_bytes, fresh on every call - its
    zeroed state is the one a process starts from).  All do what they always did while ``active`` is False.

    Not redirected: anything a wrapper allocates other than by ``torch.empty(..., device=)`` / ``torch.empty_like`` (today
    nothing: ``torch.zeros`` appears in gn_team_sync only).  run_guarded asserts that every tensor a guarded call returns
    lies inside the pool, so a wrapper that starts to allocate another way is noticed."""

    def __init__(self, ops, pool: GuardPool):
        self.ops, self.pool, self.active = ops, pool, False
        self._workspace = ops.workspace
        self._gn_team_sync = getattr(ops, "gn_team_sync", None)
        self.torch = _TorchProxy(self)
        self.workspace_calls = 0
        self.outputs_patched = False

    def workspace(self, nbytes: int, device) -> torch.Tensor:
        if not self.active:
            return self._workspace(nbytes, device)
        self.workspace_calls += 1
        t = self.pool.take_bytes(int(nbytes), f"workspace#{self.workspace_calls}({int(nbytes)} bytes)")
        assert t.numel() == int(nbytes)
        return t

    def gn_team_sync(self, device) -> torch.Tensor:
        if not self.active:
            return self._gn_team_sync(device)
        t = self.pool.take_bytes(int(self.ops.lib().psld_gn_bwd_team_sync_bytes()), "gn_team_sync")
        return t.zero_()

    def install(self, monkeypatch, outputs: bool = True):
        monkeypatch.setattr(self.ops, "workspace", self.workspace)
        if outputs:
            monkeypatch.setattr(self.ops, "torch", self.torch)
            monkeypatch.setattr(self.ops, "gn_team_sync", self.gn_team_sync)
            self.outputs_patched = True
        return self

    def __enter__(self):
        self.active = True
        return self

    def __exit__(self, *exc):
        self.active = False
        return False


# ---------------------------------------------------------------------------------------------------------------------
# one call, twice
# ---------------------------------------------------------------------------------------------------------------------
def _is_tensor(v):
    return isinstance(v, torch.Tensor)


def _parts(v):
    """The tensors inside a value: a tensor, an object carrying tensors (ops.LimbPlanes: ``t``; ops.GNStats: ``mean`` /
    ``rstd`` / ``scale`` / ``shift``), a list / tuple of those, or something without tensors."""
    if _is_tensor(v):
        return [("", v)]
    if isinstance(v, (list, tuple)):
        return [(f"[{i}]{n}", t) for i, e in enumerate(v) for n, t in _parts(e)]
    slots = [s for s in getattr(type(v), "__slots__", ()) if _is_tensor(getattr(v, s, None))]
    return [(f".{s}", getattr(v, s)) for s in slots]


def _rebuild(v, fn, name):
    """``v`` with every tensor t inside replaced by fn(t, name)."""
    if _is_tensor(v):
        return fn(v, name)
    if isinstance(v, (list, tuple)):
        return type(v)(_rebuild(e, fn, f"{name}[{i}]") for i, e in enumerate(v))
    slots = [s for s in getattr(type(v), "__slots__", ()) if _is_tensor(getattr(v, s, None))]
    if not slots:
        return v
    new = object.__new__(type(v))
    for s in type(v).__slots__:
        if hasattr(v, s):
            val = getattr(v, s)
            setattr(new, s, fn(val, f"{name}.{s}") if _is_tensor(val) else val)
    return new


def _clone(t, name):
    c = t.clone()
    for k, v in getattr(t, "__dict__", {}).items():
        setattr(c, k, v)
    return c


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _cols(t, cols):
    ld = t.shape[-1]
    lo, hi = (0, cols) if isinstance(cols, int) else cols
    assert 0 <= lo < hi <= ld, (lo, hi, ld)
    return lo, hi, ld


def _pattern_like(t, shape):
    n = _nbytes(shape, t.dtype)
    return torch.full((n,), PATTERN, dtype=torch.uint8, device=t.device).view(t.dtype).view(shape)


def _fill_gap(t, cols):
    """Pattern into the columns outside ``cols`` = (lo, hi) of every row (the last dimension is the leading dimension)."""
    lo, hi, ld = _cols(t, cols)
    rows = t.view(-1, ld)
    if lo:
        rows[:, :lo] = _pattern_like(t, (rows.shape[0], lo))
    if hi < ld:
        rows[:, hi:] = _pattern_like(t, (rows.shape[0], ld - hi))


def _gap_intact(t, cols) -> bool:
    lo, hi, ld = _cols(t, cols)
    rows = t.view(-1, ld)
    return all(bool((_bytes(g) == PATTERN).all()) for g in (rows[:, :lo], rows[:, hi:]) if g.numel())


def run_guarded(guard: Guard, fn, tensors: dict, outputs=()):
    """Call ``fn(**tensors)`` once on ordinary clones and once on guarded copies with the same contents, and assert

    (a) the ordinary outputs are finite, (b) the guarded outputs equal them under torch.equal, (c) every non-output
    tensor is unchanged after the call, bit for bit, (d) no band of the pool was touched.

    ``tensors``: name -> tensor / LimbPlanes / GNStats / list of those / anything else (passed through).  ``outputs``: the
    names ``fn`` writes - a dict ``name -> width`` (or ``name -> (lo, hi)``, or None) marks an output whose last dimension is a leading dimension
    larger than the columns the call may write: the gap columns are pattern-filled and must stay so.  Whatever ``fn`` returns
    (tensors the wrapper allocated itself) counts as output too.  Returns the ordinary run's (tensors, returned value)."""
    widths = dict(outputs) if isinstance(outputs, dict) else {n: None for n in outputs}
    for n in widths:
        assert n in tensors, n
    pool = guard.pool
    pool.release() if pool.regions else None
    guard.workspace_calls = 0

    def gapfill(kw):
        for n, wdt in widths.items():
            if wdt is not None:
                _fill_gap(kw[n], wdt)

    plain = {n: _rebuild(v, _clone, n) for n, v in tensors.items()}
    gapfill(plain)
    assert not guard.active
    ret_plain = fn(**plain)
    guarded = {n: _rebuild(v, pool.take_like, n) for n, v in tensors.items()}
    gapfill(guarded)
    with guard:
        ret_guarded = fn(**guarded)
    torch.cuda.synchronize() if pool.buf.is_cuda else None

    # (d) first: a touched band explains whatever else differs
    pool.check()
    outs_p = [(n, t, widths[n]) for n in widths for _, t in _named(n, plain[n])]
    outs_g = [(n, t, widths[n]) for n in widths for _, t in _named(n, guarded[n])]
    outs_p += [(n, t, None) for n, t in _named("returned", ret_plain)]
    outs_g += [(n, t, None) for n, t in _named("returned", ret_guarded)]
    assert len(outs_p) == len(outs_g)
    if guard.outputs_patched:            # a wrapper-owned output that did not come from the pool would go unguarded
        lo = pool.buf.data_ptr()
        for n, t in _named("returned", ret_guarded):
            assert not t.numel() or lo <= t.data_ptr() < lo + pool.buf.numel(), f"'{n}' of the guarded call is not in the pool"
    for (n, a, wdt), (_, b, _) in zip(outs_p, outs_g):
        if wdt is not None:
            lo, hi, _ = _cols(a, wdt)
        av, bv = (a, b) if wdt is None else (a[..., lo:hi], b[..., lo:hi])
        if a.is_floating_point():
            assert bool(torch.isfinite(av).all()), f"(a) output '{n}' of the ordinary call is not finite"
        if not torch.equal(av, bv):
            diff = (av != bv) | (av != av) | (bv != bv)
            idx = torch.nonzero(diff.reshape(-1))[:, 0]
            raise GuardViolation(f"(b) output '{n}' differs between ordinary and guarded buffers in {idx.numel()} of "
                                 f"{av.numel()} elements, first at flat index {int(idx[0])}: "
                                 f"{av.reshape(-1)[idx[0]].item()} vs {bv.reshape(-1)[idx[0]].item()}")
        if wdt is not None:
            assert _gap_intact(a, wdt), f"gap columns of '{n}' (ordinary buffers) were written"
            assert _gap_intact(b, wdt), f"gap columns of '{n}' (guarded buffers) were written"
    for n, v in tensors.items():
        if n in widths:
            continue
        for (sub, t0), (_, tp), (_, tg) in zip(_parts(v), _parts(plain[n]), _parts(guarded[n])):
            assert torch.equal(_bytes(tp), _bytes(t0)), f"(c) input '{n}{sub}' changed (ordinary buffers)"
            assert torch.equal(_bytes(tg), _bytes(t0)), f"(c) input '{n}{sub}' changed (guarded buffers)"
    return plain, ret_plain


def _named(name, v):
    return [(name + sub, t) for sub, t in _parts(v)] if v is not None else []


# ---------------------------------------------------------------------------------------------------------------------
# arena with bands
# ---------------------------------------------------------------------------------------------------------------------
def make_guarded_arena(ops):
    """GuardedArena(ops.Arena): every slice has exactly the bytes asked for, a 256-byte aligned start and at least 64 KiB of
    pattern on each side.  Bump allocation like the parent, so addresses repeat from step to step.  ``reset()`` counts the
    changed band bytes of the pass ON THE DEVICE (no host read) and restores the pattern over the range the pass used - on
    the stream that calls it, like every other access to arena memory; ``violations()`` reads the count - once, at the end
    of the test."""

    class GuardedArena(ops.Arena):
        instances = []

        def __init__(self, device, nbytes: int = 1 << 24):
            super().__init__(device, nbytes)
            self.buf.fill_(PATTERN)
            self.count = torch.zeros((), dtype=torch.int64, device=device)
            self.slices = []                                # (buf, start, end) handed out since the last reset
            self.total_slices = 0
            self.peak = 0                                   # bytes of one buffer in use, bands included
            GuardedArena.instances.append(self)

        def _sweep(self):
            """Count the changed bytes of every band of this pass, then restore the pattern over everything it used."""
            counts, used = [], {}
            prev_buf, prev_end = None, 0
            for buf, start, end in self.slices:
                if buf is not prev_buf:
                    if prev_buf is not None:
                        counts.append(torch.count_nonzero(prev_buf[prev_end:prev_end + ARENA_BAND] != PATTERN))
                    prev_buf, prev_end = buf, 0
                counts.append(torch.count_nonzero(buf[prev_end:start] != PATTERN))
                prev_end = end
                used[id(buf)] = (buf, min(buf.numel(), end + ARENA_BAND))
            if prev_buf is not None:
                counts.append(torch.count_nonzero(prev_buf[prev_end:prev_end + ARENA_BAND] != PATTERN))
            if counts:
                self.count += torch.stack(counts).sum()
            for buf, hi in used.values():
                self.peak = max(self.peak, hi)
                buf[:hi].fill_(PATTERN)
            self.slices = []

        def _aligned(self, off: int) -> int:
            return off + (-(self.buf.data_ptr() + off)) % ALIGN

        def reset(self):
            self._sweep()
            super().reset()

        def alloc(self, nbytes: int):
            nbytes = int(nbytes)
            start = self._aligned(self.off + ARENA_BAND)
            if start + nbytes + ARENA_BAND > self.buf.numel():
                self.high = max(self.high, self.off)
                self.retired.append(self.buf)
                size = max(2 * self.buf.numel(), 2 * ARENA_BAND + ALIGN + nbytes, 2 * self.high)
                self.buf = torch.full((size,), PATTERN, device=self.device, dtype=torch.uint8)
                start = self._aligned(ARENA_BAND)
            assert (self.buf.data_ptr() + start) % ALIGN == 0
            out = self.buf[start:start + nbytes]
            self.slices.append((self.buf, start, start + nbytes))
            self.off = start + nbytes
            self.total_slices += 1
            return out

        def violations(self) -> int:
            """Changed band bytes so far, the current pass included (a host read; the pass's slices are dead afterwards)."""
            self._sweep()
            return int(self.count.item())

    return GuardedArena
