"""A fenced, poisoned allocator for ONE call: what a kernel does with memory it did not fill itself, made a test input.

``GuardedArena`` is one uint8 tensor from the real allocator, set to a fence byte.  ``take`` carves payloads out of it, each on
a 256-byte boundary with at least ``FENCE`` fence bytes on either side, and sets the payload to a fill byte.  ``guarded(arena)``
redirects ``torch.empty``, ``torch.empty_like`` and ``torch.zeros`` on the arena's device into it, so that every scratch,
workspace, packed-weight buffer and output an entry point allocates for itself

* holds a chosen byte pattern instead of whatever the caching allocator left (0x00 flatters a kernel that needs zeroed
  scratch, 0xFF is NaN in fp16 / fp32 / fp64, -1 in every integer width, 255 in a mask), and
* ends where it was declared to end: the caching allocator rounds to 512 B, so an overrun of a few bytes lands in slack;
  here it lands in a fence, and ``damaged()`` names the allocation next to it and the Python line that made it.

An overrun stays inside the arena (memory the process owns), so nothing here provokes a fault.  An overrun longer than
``FENCE`` reaches the next payload and shows in the comparison of results instead.

``FENCE = 4096`` is a choice, not a measurement: a 256-lane row of 16-byte stores.
"""
import contextlib
import sys
from collections import namedtuple

import torch

FENCE = 4096
ALIGN = 256

# (fill byte, fence byte) of run modes a and b; mode c ("leftover") fills nothing: rewind() after a case of other extents.
MODES = {"a": (0x00, 0xA5), "b": (0xFF, 0x5A)}
LEFTOVER_FENCE = 0xC3

Allocation = namedtuple("Allocation", "start end shape dtype site")
# one damaged fence byte: its arena offset, what it holds now, the nearest allocation, which side of that allocation's payload
# it lies on ("before" / "after") and how many bytes away from the payload's first / one-past-last byte
Damage = namedtuple("Damage", "offset value allocation side distance")

_HERE = __file__[:-1] if __file__.endswith((".pyc", ".pyo")) else __file__


class ArenaExhausted(RuntimeError):
    pass


def _device(device):
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _call_site():
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == _HERE:
        f = f.f_back
    if f is None:
        return "<unknown>"
    return f"{f.f_code.co_filename}:{f.f_lineno} in {f.f_code.co_name}"


class GuardedArena:
    def __init__(self, nbytes, device, fill, fence):
        """``fill``: the byte every payload is set to, or None to leave it as it is (leftover mode)."""
        self.device = _device(device)
        self.fill, self.fence = fill, int(fence)
        assert 0 <= self.fence < 256 and (fill is None or 0 <= int(fill) < 256)
        self._empty = torch.empty                              # the real allocator: nothing is patched yet
        raw = self._empty(int(nbytes) + ALIGN, dtype=torch.uint8, device=self.device)
        raw.fill_(self.fence)
        skew = -raw.data_ptr() % ALIGN
        self.buf = raw[skew:skew + int(nbytes)]
        self.size = int(nbytes)
        self.ptr = 0              # one past the last payload
        self.stale = 0            # bytes [ptr, stale) hold what the run before rewind() left: neither payload nor fence
        self.allocations = []
        self.served = 0           # allocations since construction, rewinds included

    def take(self, shape, dtype):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            if s < 0:
                raise ValueError(f"GuardedArena.take: negative extent in {shape}")
            n *= s
        nbytes = n * _itemsize(dtype)
        start = (self.ptr + FENCE + ALIGN - 1) // ALIGN * ALIGN
        end = start + nbytes
        if end + FENCE > self.size:
            raise ArenaExhausted(f"GuardedArena: {nbytes} bytes for {shape} {dtype} at {_call_site()} do not fit: "
                                 f"{self.size - self.ptr} of {self.size} bytes left (with {FENCE} fence bytes on either side)")
        if self.stale > self.ptr:                       # after rewind(): lay the fences of this payload over the leftovers
            self.buf[self.ptr:start].fill_(self.fence)
            self.buf[end:end + FENCE].fill_(self.fence)
            if self.stale <= end + FENCE:
                self.stale = 0
        payload = self.buf[start:end]
        if self.fill is not None:
            payload.fill_(int(self.fill))
        self.ptr = end
        self.allocations.append(Allocation(start, end, shape, dtype, _call_site()))
        self.served += 1
        # a tensor of its own on the arena's storage, not a view of the arena: like a fresh allocation it has no base and its own
        # version counter (autograd refuses custom-Function outputs that are views of a tensor modified in place)
        t = self._empty(0, dtype=dtype, device=self.device)
        offset = self.buf.storage_offset() + start
        assert offset % _itemsize(dtype) == 0
        return t.set_(self.buf.untyped_storage(), offset // _itemsize(dtype), shape)

    def rewind(self):
        """Start over at offset 0 and refill nothing: the next run's payloads hold what this one left ("leftover" mode).
        ``take`` lays each new payload's fences as it goes; what lies beyond them is not looked at until it is fenced again."""
        self.stale = max(self.stale, min(self.size, self.ptr + FENCE))
        self.ptr = 0
        self.allocations = []

    def damaged(self):
        """Every byte outside the payloads that is no longer the fence byte, as ``Damage`` rows in offset order."""
        bad = self.buf != self.fence
        for a in self.allocations:
            bad[a.start:a.end] = False
        if self.stale > self.ptr + FENCE:
            bad[self.ptr + FENCE:self.stale] = False
        offsets = bad.nonzero().flatten().cpu().tolist()
        if not offsets:
            return []
        values = self.buf.cpu()
        out = []
        for off in offsets:
            best = None
            for a in self.allocations:
                side, dist = ("before", a.start - off) if off < a.start else ("after", off - a.end + 1)
                if best is None or dist < best[2]:
                    best = (a, side, dist)
            a, side, dist = best if best is not None else (None, None, None)
            out.append(Damage(off, int(values[off]), a, side, dist))
        return out

    def describe_damage(self, limit=8):
        rows = self.damaged()
        lines = [f"{len(rows)} fence byte(s) damaged"]
        for r in rows[:limit]:
            a = r.allocation
            where = "no allocation" if a is None else f"{r.distance} byte(s) {r.side} {a.shape} {a.dtype} from {a.site}"
            lines.append(f"  offset {r.offset}: 0x{r.value:02x} (fence 0x{self.fence:02x}), {where}")
        return "\n".join(lines)


def _itemsize(dtype):
    return torch._utils._element_size(dtype)         # not torch.empty(()).element_size(): torch.empty may be the patched one


class _Patch:
    """What ``guarded`` hands back: ``passed_through`` counts allocations on the arena's device that it could not redirect."""

    def __init__(self, arena):
        self.arena = arena
        self.passed_through = 0
        self.passed_sites = []

    def _pass(self, what):
        self.passed_through += 1
        self.passed_sites.append(f"{what} at {_call_site()}")


def _size_of(args, kwargs):
    if "size" in kwargs:
        size = kwargs.pop("size")
    elif len(args) == 1 and not isinstance(args[0], int):
        size = args[0]
    else:
        size = args
    if isinstance(size, torch.Tensor):
        return None
    try:
        return tuple(int(s) for s in size)
    except (TypeError, ValueError):
        return None


_PLAIN = {"dtype", "device", "requires_grad", "pin_memory", "layout", "memory_format", "out", "names"}


def _plain_kwargs(kw):
    """True when the keywords ask for nothing but an ordinary contiguous strided tensor."""
    return (set(kw) <= _PLAIN and kw.get("out") is None and not kw.get("requires_grad", False) and not kw.get("pin_memory", False)
            and kw.get("layout", torch.strided) == torch.strided and kw.get("names") is None
            and kw.get("memory_format", torch.contiguous_format) == torch.contiguous_format)


@contextlib.contextmanager
def guarded(arena, ops=None, holders=()):
    """Redirect ``torch.empty``, ``torch.empty_like`` and ``torch.zeros`` on ``arena.device`` into ``arena`` for the block.

    ``ops``: the package's ops module; its grow-only cached workspaces (``_WGRAD_WS``, ``_SPLITK_WS``, ``_GEMM_WS``, and the
    retired list that goes with them) are swapped for empty ones, so they are allocated again, inside the arena.  ``_ZERO_BIAS``
    and ``_TEMB_FREQS`` are filled by the wrapper and read-only afterwards: they stay.
    ``holders``: objects that cache a ``_scratch`` tensor (augment.IntensityAugmenter; a DeviceBatchProducer is followed to its
    ``intensity``): it is dropped for the block and put back afterwards."""
    real_empty, real_empty_like, real_zeros = torch.empty, torch.empty_like, torch.zeros
    state = _Patch(arena)

    def wants(device):
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        try:
            return _device(device) == arena.device
        except (RuntimeError, TypeError):
            return False

    def new(real, name, args, kwargs, zero):
        if not wants(kwargs.get("device")):
            return real(*args, **kwargs)
        kw = dict(kwargs)
        size = _size_of(args, kw)
        if size is None or not _plain_kwargs(kw):
            state._pass(name)
            return real(*args, **kwargs)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        t = arena.take(size, dtype)
        return t.zero_() if zero else t

    def empty(*args, **kwargs):
        return new(real_empty, "torch.empty", args, kwargs, False)

    def zeros(*args, **kwargs):
        return new(real_zeros, "torch.zeros", args, kwargs, True)

    def empty_like(t, *args, **kwargs):
        if not isinstance(t, torch.Tensor) or not wants(kwargs.get("device", t.device)):
            return real_empty_like(t, *args, **kwargs)
        fmt = kwargs.get("memory_format", torch.preserve_format)
        plain = (not args and set(kwargs) <= _PLAIN and t.layout == torch.strided and t.is_contiguous()
                 and fmt in (torch.preserve_format, torch.contiguous_format) and not kwargs.get("requires_grad", False)
                 and not kwargs.get("pin_memory", False) and kwargs.get("layout", torch.strided) == torch.strided)
        if not plain:
            state._pass("torch.empty_like")
            return real_empty_like(t, *args, **kwargs)
        return arena.take(tuple(t.shape), kwargs.get("dtype") or t.dtype)

    swapped = []
    if ops is not None:
        for name, fresh in (("_WGRAD_WS", {}), ("_SPLITK_WS", {}), ("_GEMM_WS", {}), ("_WGRAD_WS_RETIRED", [])):
            if hasattr(ops, name):
                swapped.append((ops, name, getattr(ops, name)))
                setattr(ops, name, fresh)
    for h in holders:
        for obj in (h, getattr(h, "intensity", None)):
            if obj is not None and "_scratch" in getattr(obj, "__dict__", {}):
                swapped.append((obj, "_scratch", obj._scratch))
                obj._scratch = None
    torch.empty, torch.empty_like, torch.zeros = empty, empty_like, zeros
    try:
        yield state
    finally:
        torch.empty, torch.empty_like, torch.zeros = real_empty, real_empty_like, real_zeros
        for obj, name, old in reversed(swapped):
            setattr(obj, name, old)
