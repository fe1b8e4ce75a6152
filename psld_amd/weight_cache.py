"""Derived copies of a network's weights (packed layouts, bf16 limb / Winograd fragments, gathered biases and
projections), refreshed in place when their parameters change.

An entry is derived from one OWNER parameter and is stale once the owner's stamp - (cache epoch, ``_version``,
``data_ptr``) - moved: an in-place write, ``invalidate()`` after writes through raw pointers (fused optimiser, EMA), or
moved storage.  Refreshes are lazy and write into the existing buffers (captured hipGraphs hold their addresses).  The
first stale access of an entry in a batch FAMILY refreshes every entry of the family with ONE launch over a device
table (rebuilt only when the entries or their pointers change), provided the family has ``min_entries`` entries; a new
entry, or one whose family cannot batch, is built on its own.  Launchers and builders come from the caller.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch


def _first(out) -> torch.Tensor:
    return out[0] if isinstance(out, tuple) else out


class Entry:
    """``out``: the buffer (or tuple of buffers) kernels read.  ``build(prev)`` rebuilds the entry alone, refilling
    ``prev`` in place (None: allocate), and returns ``out``; an entry only its family refreshes is made with ``out``
    allocated and no ``build``.  ``rows(out)``: its (table row, work items) pairs in the family launch.  ``graph``: the
    replayed inference forward reads it (``WeightCache.refresh``)."""

    __slots__ = ("owner", "out", "build", "family", "rows", "graph", "stamp")

    def __init__(self, owner: torch.Tensor, out=None, build: Optional[Callable] = None, family: Optional[str] = None,
                 rows: Optional[Callable] = None, graph: bool = False):
        self.owner, self.out, self.build, self.family, self.rows, self.graph = owner, out, build, family, rows, graph
        self.stamp = None


class _Family:
    __slots__ = ("launch", "min_entries", "members", "table")

    def __init__(self, launch: Callable, min_entries: int):
        self.launch, self.min_entries = launch, min_entries
        self.members: List[Entry] = []
        self.table = None       # (signature, device table, rows, total work items)


class WeightCache:
    """``families``: name -> (``launch(table, rows, total work items)``, entries needed for a batched refresh)."""

    def __init__(self, families: Dict[str, Tuple[Callable, int]]):
        self.families = {name: _Family(launch, n) for name, (launch, n) in families.items()}
        self.entries: Dict[tuple, Entry] = {}
        self.epoch = 0

    def stamp(self, p: torch.Tensor):
        return (self.epoch, p._version, p.data_ptr())

    def invalidate(self):
        self.epoch += 1

    def clear(self):
        """Forget every entry (the parameters moved to new storage)."""
        self.entries.clear()
        for f in self.families.values():
            f.members.clear()
            f.table = None
        self.epoch += 1

    def entry(self, owner: torch.Tensor, tag: str, make: Callable, *args) -> Entry:
        """The entry (owner, tag), made by ``make(owner, *args)`` and built on first use; not refreshed."""
        e = self.entries.get((id(owner), tag))
        if e is None:
            e = make(owner, *args)
            if e.out is None:
                e.out = e.build(None)
                e.stamp = self.stamp(owner)
            self.entries[(id(owner), tag)] = e
            if e.family is not None:
                f = self.families[e.family]
                f.members.append(e)
                f.table = None
        return e

    def get(self, owner: torch.Tensor, tag: str, make: Callable, *args):
        """The fresh buffer(s) of the entry (owner, tag)."""
        e = self.entries.get((id(owner), tag))
        if e is not None and e.stamp == self.stamp(owner):
            return e.out
        return self.fresh(e if e is not None else self.entry(owner, tag, make, *args))

    def fresh(self, e: Entry):
        """``e.out``, refreshed first if stale."""
        if e.stamp == self.stamp(e.owner):
            return e.out
        f = self.families.get(e.family)
        if f is not None and self._batch(f):
            return e.out
        e.out = e.build(e.out if _first(e.out).device == e.owner.device else None)
        e.stamp = self.stamp(e.owner)
        if f is not None:
            f.table = None
        return e.out

    def refresh(self, forward_only: bool = True):
        """Refresh, in registration order, every stale entry (``forward_only``: every one marked ``graph``)."""
        for e in list(self.entries.values()):
            if e.graph or not forward_only:
                self.fresh(e)

    def _batch(self, f: _Family) -> bool:
        """Refresh every entry of ``f`` with one launch; False when there is nothing to batch."""
        es = f.members
        if len(es) < f.min_entries or any(_first(e.out).device != e.owner.device for e in es):
            return False
        sig = tuple((e, e.owner.data_ptr(), _first(e.out).data_ptr()) for e in es)
        if f.table is None or f.table[0] != sig:
            rows, total = [], 0
            for e in es:
                for row, items in e.rows(e.out):
                    rows.append(row + [total])
                    total += items
            f.table = (sig, torch.tensor(rows, dtype=torch.int64, device=es[0].owner.device), len(rows), total)
        _, table, n, total = f.table
        f.launch(table, n, total)
        for e in es:
            e.stamp = self.stamp(e.owner)
        return True
