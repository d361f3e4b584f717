"""tests/guarded_alloc.py on the CPU: the arena finds a one-byte overrun and names its allocation, the two fill modes tell a
read-before-write apart, other devices pass through, the patch leaves with an exception, exhaustion raises and never falls
back, and torch.nn.functional is unaffected."""
import pytest
import torch

import guarded_alloc as GA


def _overrun_by_one():
    t = torch.empty(100, dtype=torch.uint8)                   # <- the allocation the report has to name
    t.fill_(7)
    torch.as_strided(t, (101,), (1,))[100] = 9                # one byte past the end: inside the arena, in the fence
    return t


def _reads_before_writing():
    acc = torch.empty(8, dtype=torch.float32)
    acc += 1.0                                                # needs zeroed scratch
    return acc


def _arena(mode, nbytes=1 << 16, device="cpu"):
    fill, fence = GA.MODES[mode]
    return GA.GuardedArena(nbytes, device, fill, fence)


def test_one_byte_overrun_is_reported_with_its_call_site():
    arena = _arena("a")
    with GA.guarded(arena) as g:
        before = torch.empty((3, 5), dtype=torch.float64)
        t = _overrun_by_one()
        after = torch.empty(4, dtype=torch.int32)
    assert g.passed_through == 0 and arena.served == 3
    assert torch.equal(t, torch.full((100,), 7, dtype=torch.uint8))
    rows = arena.damaged()
    assert len(rows) == 1
    (r,) = rows
    assert r.value == 9 and r.side == "after" and r.distance == 1
    assert r.allocation.shape == (100,) and r.allocation.dtype == torch.uint8
    assert "test_guarded_alloc.py" in r.allocation.site and "_overrun_by_one" in r.allocation.site
    assert r.offset == r.allocation.end
    assert "_overrun_by_one" in arena.describe_damage()
    del before, after


def test_underrun_is_reported_before_its_allocation():
    arena = _arena("b")
    with GA.guarded(arena):
        t = torch.empty(16, dtype=torch.float32)
        torch.as_strided(t, (1,), (1,), t.storage_offset() - 1).fill_(0.0)
    rows = arena.damaged()
    assert [r.side for r in rows] and all(r.side == "before" and r.allocation.shape == (16,) for r in rows)
    assert len(rows) == 4 and sorted(r.distance for r in rows) == [1, 2, 3, 4]


def test_layout_alignment_fences_and_fill():
    arena = _arena("b")
    with GA.guarded(arena):
        a = torch.empty(3, 7, dtype=torch.float16)
        b = torch.zeros((2, 2), dtype=torch.int64)
        c = torch.empty_like(a, dtype=torch.float32)
        d = torch.empty(size=(5,), dtype=torch.uint8, device="cpu")
        e = torch.empty(0, dtype=torch.float32)
    assert a.shape == (3, 7) and c.shape == (3, 7) and c.dtype == torch.float32 and d.shape == (5,) and e.numel() == 0
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(c).all()) and bool((d == 255).all())        # 0xFF: NaN, 255
    assert bool((b == 0).all())                                                                       # zeros: take, then zero
    allocs = arena.allocations
    assert len(allocs) == 5
    prev_end = 0
    for al in allocs:
        assert al.start % GA.ALIGN == 0 and al.start - prev_end >= GA.FENCE
        assert (arena.buf.data_ptr() + al.start) % GA.ALIGN == 0
        prev_end = al.end
    assert arena.size - prev_end >= GA.FENCE
    assert arena.damaged() == []
    a.fill_(1.0); b.fill_(-1); c.fill_(2.0); d.fill_(3)        # writing every payload to its last byte damages nothing
    assert arena.damaged() == []


def test_read_before_write_differs_between_modes():
    out = {}
    for mode in ("a", "b"):
        arena = _arena(mode)
        with GA.guarded(arena):
            out[mode] = _reads_before_writing().clone()
        assert arena.damaged() == []
    assert torch.equal(out["a"], torch.ones(8))
    assert not torch.equal(out["a"].view(torch.uint8), out["b"].view(torch.uint8))


def test_leftover_mode_keeps_what_the_run_before_left():
    arena = GA.GuardedArena(1 << 16, "cpu", None, GA.LEFTOVER_FENCE)
    with GA.guarded(arena):
        torch.empty(3000, dtype=torch.uint8).fill_(17)
        torch.empty(5000, dtype=torch.uint8).fill_(19)
        assert arena.damaged() == []
        arena.rewind()
        t = torch.empty(9000, dtype=torch.uint8)               # spans the first payload, its fence and part of the second
        u = torch.empty(100, dtype=torch.uint8)
    seen = set(t.unique().tolist())
    assert 17 in seen and 19 in seen                           # the leftovers, not a fill
    assert arena.damaged() == []                               # the new payloads' fences were laid over the leftovers
    torch.as_strided(u, (101,), (1,))[100] = 1
    assert [(r.side, r.distance, r.allocation.shape) for r in arena.damaged()] == [("after", 1, (100,))]


def test_other_devices_pass_through():
    arena = GA.GuardedArena.__new__(GA.GuardedArena)            # an arena that claims another device type, without needing one
    GA.GuardedArena.__init__(arena, 1 << 14, "cpu", 0xFF, 0x5A)
    arena.device = torch.device("meta")
    with GA.guarded(arena) as g:
        a = torch.empty(10, dtype=torch.float32)
        b = torch.zeros(10, dtype=torch.float32, device="cpu")
        c = torch.empty_like(a)
    assert arena.served == 0 and g.passed_through == 0          # not this arena's device: neither redirected nor counted
    assert bool((b == 0).all()) and c.shape == a.shape
    assert not bool((arena.buf != 0x5A).any())


def test_forms_it_cannot_redirect_are_counted():
    arena = _arena("a")
    with GA.guarded(arena) as g:
        torch.empty_like(torch.ones(4, 6).t())                  # non-contiguous: a stride-preserving empty_like
        torch.empty(4, out=torch.ones(4))
        torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
    assert g.passed_through == 3 and arena.served == 0
    assert all("test_forms_it_cannot_redirect_are_counted" in s for s in g.passed_sites)


def test_patch_is_gone_after_an_exception():
    real = (torch.empty, torch.empty_like, torch.zeros)
    arena = _arena("a")
    with pytest.raises(KeyError):
        with GA.guarded(arena):
            assert torch.empty is not real[0]
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.zeros) == real
    torch.empty(4)
    assert arena.served == 0


def test_cached_workspaces_are_swapped_and_put_back():
    class Ops:
        pass

    class Holder:
        def __init__(self):
            self._scratch = "old"

    class Producer:
        def __init__(self):
            self.intensity = Holder()

    ops, h, p = Ops(), Holder(), Producer()
    ops._WGRAD_WS, ops._SPLITK_WS, ops._GEMM_WS, ops._WGRAD_WS_RETIRED = {"k": 1}, {"k": 2}, {"k": 3}, [4]
    ops._ZERO_BIAS = keep = {"z": 0}
    with pytest.raises(ValueError):
        with GA.guarded(_arena("a"), ops=ops, holders=(h, p)):
            assert ops._WGRAD_WS == {} and ops._SPLITK_WS == {} and ops._GEMM_WS == {} and ops._WGRAD_WS_RETIRED == []
            assert ops._ZERO_BIAS is keep
            assert h._scratch is None and p.intensity._scratch is None
            ops._GEMM_WS["new"] = 1
            raise ValueError
    assert (ops._WGRAD_WS, ops._SPLITK_WS, ops._GEMM_WS, ops._WGRAD_WS_RETIRED) == ({"k": 1}, {"k": 2}, {"k": 3}, [4])
    assert h._scratch == "old" and p.intensity._scratch == "old"


def test_exhaustion_raises_and_never_falls_back():
    arena = _arena("a", nbytes=3 * GA.FENCE)
    with GA.guarded(arena):
        torch.empty(GA.FENCE - 512, dtype=torch.uint8)
        with pytest.raises(GA.ArenaExhausted):
            torch.empty(1024, dtype=torch.uint8)
        with pytest.raises(GA.ArenaExhausted):
            torch.zeros(1 << 20, dtype=torch.float32)
    assert arena.served == 1


def test_functional_conv3d_is_unaffected():
    g = torch.Generator().manual_seed(0)
    x, w, b = torch.randn(1, 2, 5, 6, 7, generator=g), torch.randn(3, 2, 3, 3, 3, generator=g), torch.randn(3, generator=g)
    want = torch.nn.functional.conv3d(x, w, b, padding=1)
    for mode in ("a", "b"):
        arena = _arena(mode)
        with GA.guarded(arena):
            got = torch.nn.functional.conv3d(x, w, b, padding=1)
        assert torch.equal(got, want)
        assert arena.damaged() == []


@pytest.mark.gpu
def test_on_the_device_a_read_before_write_and_an_overrun_are_seen():
    """The same two defects with the arena on the GPU, in torch operators: what the buffer-contract tests rely on."""
    out = {}
    for mode in ("a", "b"):
        arena = _arena(mode, device="cuda")
        with GA.guarded(arena) as g:
            acc = torch.empty(8, dtype=torch.float32, device="cuda")
            acc += 1.0
            t = torch.zeros(100, dtype=torch.uint8, device="cuda:0")
            host = torch.empty(3)                                   # another device: not this arena's
            torch.cuda.synchronize()
            assert arena.damaged() == []
            torch.as_strided(t, (101,), (1,))[100] = 9              # inside the arena: the process owns the byte
            torch.cuda.synchronize()
        assert g.passed_through == 0 and arena.served == 2 and not host.is_cuda
        (r,) = arena.damaged()
        assert (r.value, r.side, r.distance, r.allocation.shape) == (9, "after", 1, (100,))
        assert "test_on_the_device" in r.allocation.site
        out[mode] = acc.cpu()
    assert torch.equal(out["a"], torch.ones(8)) and bool(torch.isnan(out["b"]).all())
