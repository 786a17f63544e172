"""The plumbing every device feed shares: the layout of ONE ``uint8`` device arena, the ring of pinned host slots a
transfer goes through, and the recipe buffer of the device-side builders (``CLSRNet.upload`` / ``build_feed`` /
``build_eval_feed`` are its callers; csrc/feed.hip holds the kernels).

A device feed is a dict: the scalars ``B, T, compact, G``, a tensor per name of its spec (views into the arena) and two
private entries, ``_arena`` (:class:`Arena`) and, on feeds of ``build_feed``, ``_rbuf`` (:class:`RecipeBuffer`).  A feed
passed back through ``into=`` NEVER gets a new arena: captured graphs and the launch plan hold its addresses.  Only the
recipe buffer may be reallocated."""
import math

import numpy as np
import torch

from clsr_amd import ops

I32, F32 = torch.int32, torch.float32


def length_threshold(hp):
    """Histories longer than this count into ``denom`` (unset for the sibling models: 0)."""
    return getattr(hp, "contrastive_length_threshold", None) or 0


def layout(spec):
    """``spec``: a sequence of ``(name, shape, dtype)`` of 4-byte words -> ``({name: (offset, nbytes)}, total_bytes)``:
    the pieces in the order given, each on a 16-byte boundary."""
    lay, off = {}, 0
    for name, shape, _ in spec:
        nb = 4 * math.prod(shape)
        lay[name] = (off, nb)
        off += (nb + 15) // 16 * 16
    return lay, off


def train_spec(R, B, T, per_position=False):
    """``B`` rows over ``R`` history rows (``R = B / G``: compact); ``per_position``: a target per step (NextItNet)."""
    per = (B, T) if per_position else (B,)
    return (("users", (R,), I32), ("items", per, I32), ("cates", per, I32), ("item_history", (R, T), I32),
            ("item_cate_history", (R, T), I32), ("time_from_first_action", (R, T), F32), ("time_to_now", (R, T), F32),
            ("labels", (math.prod(per),), F32), ("seq_len", (R,), I32), ("denom", (1,), F32))


def eval_spec(H, n, T, users_rows):
    """A scoring feed of ``n`` lines over ``H`` history rows; ``users_rows``: the user of every line (``H < n``)."""
    s = train_spec(H, n, T)
    return s[:8] + ((("users_rows", (n,), I32),) if users_rows else ()) + s[8:]


def _stage(dev, pin, nbytes):
    """pinned -> device by ``clsr_stage_feed``, an ordinary launch on the current stream; its completion event."""
    ops.call("clsr_stage_feed", dev, pin.data_ptr(), nbytes)
    ev = torch.cuda.Event()
    ev.record()
    return ev


class PinnedRing(object):
    """Pinned host buffers of ``nbytes`` used in turn, an event per slot: a slot is never rewritten or released while a
    queued kernel reads it over PCIe."""
    _STAGE_SLOTS = 3

    def __init__(self, nbytes=0):
        self.nbytes, self._slots, self._next, self._cur = nbytes, [None] * self._STAGE_SLOTS, 0, 0

    def slot(self):
        """The next slot as ``(pinned tensor, its numpy view)``, once the transfer that last read it has completed."""
        i = self._cur = self._next
        self._next = (i + 1) % self._STAGE_SLOTS
        if self._slots[i] is None:
            pin = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)
            self._slots[i] = [pin, None, pin.numpy()]
        pin, ev, pin_np = self._slots[i]
        if ev is not None:
            ev.synchronize()
        return pin, pin_np

    def sent(self, ev):
        """``ev``: recorded after the transfer that reads the slot handed out last."""
        self._slots[self._cur][1] = ev

    def grow(self, nbytes):
        """Slots of ``nbytes`` from now on.  Every outstanding event is synchronised FIRST: only then are the old slots
        (and, by the caller, the device buffer they fed) let go of."""
        for st in self._slots:
            if st is not None and st[1] is not None:
                st[1].synchronize()
        self.nbytes, self._slots = nbytes, [None] * self._STAGE_SLOTS


class Arena(object):
    """The device side of a feed: ``dev`` (uint8), ``lay`` / ``nbytes`` (:func:`layout`), the pinned ring of ``upload``
    and ``ptrs``, the pointer descriptor a builder cached for the column store ``cols`` (compared by identity)."""

    def __init__(self, dev, lay, nbytes):
        self.dev, self.lay, self.nbytes, self.ring, self.cols, self.ptrs = dev, lay, nbytes, PinnedRing(nbytes), None, None

    def send(self, h, copy_stream=None, free=None):
        """Host arrays ``h`` (the arena's spec) -> the arena, through a pinned slot; the transfer's completion event.
        ``copy_stream``: one asynchronous copy there, after ``free`` (the event behind the last launch that reads the
        arena), in place of the staging kernel on the current stream."""
        pin, pin_np = self.ring.slot()
        for k, arr in h.items():
            o, n = self.lay[k]
            assert arr.nbytes == n
            # plain single-threaded memcpy on purpose: a torch CPU copy_ wakes the whole OpenMP pool,
            # whose spinning workers were measured to stall this thread's kernel launches for ~7 ms/step
            np.copyto(pin_np[o:o + n], arr.reshape(-1).view(np.uint8))
        if copy_stream is None:
            ev = _stage(self.dev, pin, self.nbytes)
        else:
            if free is not None:
                copy_stream.wait_event(free)
            with torch.cuda.stream(copy_stream):
                self.dev.copy_(pin, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
        self.ring.sent(ev)
        return ev


def device_feed(spec, device, B, T, compact, G):
    """A new device feed: the public scalars and a view per piece of ``spec`` into one fresh arena."""
    lay, nbytes = layout(spec)
    dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
    f = {"B": B, "T": T, "compact": compact, "G": G, "_arena": Arena(dev, lay, nbytes)}
    for k, shape, dt in spec:
        o, nb = lay[k]
        f[k] = dev[o:o + nb].view(dt).view(shape)
    return f


class RecipeBuffer(object):
    """The recipe of ``build_feed`` on its way across PCIe: a growing pinned ring, its device copy (+ scratch words)."""

    def __init__(self, device):
        self.device, self.ring, self.dev = device, PinnedRing(), None

    def send(self, sel, src, scratch=0):
        """int32 host arrays ``sel``, ``src`` -> the device on the current stream, each on a 16-byte boundary; their
        device addresses, then that of ``scratch`` bytes (never staged).  (No ``layout`` here: this runs per batch.)"""
        src_off = (sel.nbytes + 15) // 16 * 16
        nbytes = src_off + (src.nbytes + 15) // 16 * 16
        if nbytes > self.ring.nbytes:
            self.ring.grow(nbytes)
            self.dev = torch.empty(nbytes + scratch, dtype=torch.uint8, device=self.device)
        pin, pin_np = self.ring.slot()
        np.copyto(pin_np[:sel.nbytes], sel.view(np.uint8))
        np.copyto(pin_np[src_off:src_off + src.nbytes], src.reshape(-1).view(np.uint8))
        self.ring.sent(_stage(self.dev, pin, nbytes))
        base = self.dev.data_ptr()
        return base, base + src_off, base + self.ring.nbytes
