"""The three runs of one case for the buffer-contract tests (tests/test_buffer_contract_*_gpu.py), on tests/guarded_alloc.py.

mode a: every allocation the entry point makes for itself holds 0x00, fences 0xA5
mode b: 0xFF (NaN in fp16 / fp32 / fp64, -1 in every integer width, 255 in a mask), fences 0x5A
mode c: "leftover": a case of the same family with other extents runs first in the arena, then rewind() and the case under
        test over whatever that one left; fences 0xC3

``run_modes`` asserts what needs no reference: the fences are whole after torch.cuda.synchronize(), the arena served at least
one allocation, and nothing on the device was allocated past it.  The caller checks the results against the family's
reference (``same_bits`` / its own check per mode).
"""
import torch

import guarded_alloc as GA

DEVICE = "cuda"


def _detach(out):
    """A copy of every result tensor outside the arena (made with the real allocator, after the block)."""
    if torch.is_tensor(out):
        return out.clone()
    if isinstance(out, dict):
        return {k: _detach(v) for k, v in out.items()}
    if isinstance(out, (tuple, list)):
        return type(out)(_detach(v) for v in out)
    return out


def _run(arena, fn, ops, holders, what):
    with GA.guarded(arena, ops=ops, holders=holders) as g:
        out = fn()
        torch.cuda.synchronize()
        served = arena.served
        bad = arena.damaged()
        assert bad == [], f"{what}: {arena.describe_damage()}"
    assert g.passed_through == 0, f"{what}: device allocations the arena did not serve: {g.passed_sites}"
    return out, served


def run_modes(case, leftover, arena_bytes=64 << 20, holders=(), leftover_holders=()):
    """``case()`` -> a tensor, or a dict / tuple of tensors: the entry point under test on operands built OUTSIDE (everything it
    allocates inside goes to the arena).  ``leftover()``: a case of the same family with other extents.  Returns
    ({"a": out, "b": out, "c": out}, {"a": served, ...}); every out is a copy outside the arena."""
    from diff_unet_amos_amd import ops
    # ops._ZERO_BIAS is filled by the wrapper on first use and read-only afterwards (one shared vector per device spelling): it
    # is made here, by the real allocator -- made inside the block it would be a view of an arena that is rewound and dropped
    for dev in (torch.device(DEVICE), torch.device(DEVICE, torch.cuda.current_device())):
        ops.zero_bias(4096, dev)
    outs, served = {}, {}
    for mode, (fill, fence) in GA.MODES.items():
        arena = GA.GuardedArena(arena_bytes, DEVICE, fill, fence)
        out, served[mode] = _run(arena, case, ops, holders, f"mode {mode}")
        outs[mode] = _detach(out)
        del out, arena
    arena = GA.GuardedArena(arena_bytes, DEVICE, None, GA.LEFTOVER_FENCE)
    before = arena.served
    _run(arena, leftover, ops, leftover_holders, "mode c, the run that leaves its buffers behind")
    assert arena.served > before
    arena.rewind()
    before = arena.served
    out, total = _run(arena, case, ops, holders, "mode c")
    served["c"] = total - before
    outs["c"] = _detach(out)
    print(f"arena allocations served per mode: {served}")
    for mode, n in served.items():
        assert n >= 1, f"mode {mode}: the arena served no allocation: the run controlled no buffer"
    return outs, served


def _flat(out, prefix=""):
    if torch.is_tensor(out):
        yield prefix or "out", out
    elif isinstance(out, dict):
        for k, v in out.items():
            yield from _flat(v, f"{prefix}.{k}" if prefix else str(k))
    elif isinstance(out, (tuple, list)):
        for i, v in enumerate(out):
            yield from _flat(v, f"{prefix}[{i}]")


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8) if t.numel() else t.new_empty(0, dtype=torch.uint8)


def same_bits(outs, only=None, unspecified=None):
    """Results of modes a, b and c are byte-equal (NaNs included).  ``only``: the result names the promise covers (default all).
    ``unspecified``: {name: (fn(result, all results of that mode) -> bool mask of the elements the header leaves unspecified,
    citation)}: those elements are set to 0 on every side before the comparison; a mask that covers a whole tensor is refused."""
    ref = dict(_flat(outs["a"]))
    for mode in ("b", "c"):
        got = dict(_flat(outs[mode]))
        assert got.keys() == ref.keys()
        for name in ref:
            if only is not None and name not in only:
                continue
            x, y = ref[name], got[name]
            assert x.shape == y.shape and x.dtype == y.dtype, name
            if unspecified and name in unspecified:
                fn, _cite = unspecified[name]
                mx, my = fn(x, outs["a"]), fn(y, outs[mode])
                assert torch.equal(mx, my), f"{name}: the unspecified region itself differs between modes a and {mode}"
                assert x.numel() == 0 or not bool(mx.all()), f"{name}: the table may not exempt a whole tensor"
                x, y = x.clone(), y.clone()
                x[mx] = 0
                y[my] = 0
            bx, by = _bytes(x), _bytes(y)
            if not torch.equal(bx, by):
                n = int((bx != by).sum())
                first = int((bx != by).nonzero()[0]) // max(1, x.element_size())
                raise AssertionError(f"{name}: modes a and {mode} differ in {n} byte(s), first at element {first} of {tuple(x.shape)} "
                                     f"{x.dtype}: {x.reshape(-1)[first].item()} vs {y.reshape(-1)[first].item()}")
