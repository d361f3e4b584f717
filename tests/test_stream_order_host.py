"""tests/stream_order.py on synthetic traces, without a device: the region algebra, the vector clocks, every hazard kind reported and
then silenced by its ordering edge, a miniature of the Swin plan's two-stream step that passes and fails in the expected place when
any one of its three waits is deleted, and the recorder's two refusals (an unclassified tensor argument, a native launch outside a
wrapped function)."""
import ctypes
import types

import pytest
import torch

import stream_order as so
from stream_order import Region, analyse, host_barrier, launch, record, wait_event, wait_stream

MAIN, SIDE, THIRD = 0, 0x51de, 0x3d


# ---- regions -----------------------------------------------------------------------------------------------------------------------
def _cl(N=2, vox=27, Cs=32, dtype=torch.float16):
    return torch.zeros((N, 3, 3, vox // 9, Cs), dtype=dtype)


def test_channel_halves_of_a_concat_buffer_do_not_conflict():
    cat = _cl()
    up, skip = Region.channels(cat, 0, 16), Region.channels(cat, 16, 16)
    assert not up.conflicts(skip) and not skip.conflicts(up)
    assert up.conflicts(up) and up.conflicts(Region.of_tensor(cat)) and Region.of_tensor(cat).conflicts(skip)
    assert up.conflicts(Region.channels(cat, 8, 16)) and Region.channels(cat, 8, 16).conflicts(skip)      # overlapping slices
    assert not Region.channels(cat, 0, 8).conflicts(Region.channels(cat, 8, 8))                            # neighbours
    one = Region.channels(cat, 15, 1)                                                                      # one channel
    assert one.conflicts(up) and not one.conflicts(skip)


def test_a_slice_of_a_slice_and_a_strided_view_are_exact():
    cat = _cl()
    view = cat[..., 16:]                                                   # a channel slice as torch hands it on
    assert Region.of_tensor(view) == Region.channels(cat, 16, 16)
    assert Region.channels(view, 8, 8) == Region.channels(cat, 24, 8)
    rows = cat.view(-1, 32)[:, :8]                                         # the [tokens, K] operand of a GEMM with a row stride
    assert Region.of_tensor(rows) == Region.channels(cat, 0, 8)
    assert not Region.of_tensor(rows).conflicts(Region.channels(cat, 8, 24))
    odd = cat.permute(0, 4, 1, 2, 3)                                       # arbitrary strides: the hull, marked inexact
    r = Region.of_tensor(odd)
    assert not r.exact and r.hull() == Region.of_tensor(cat).hull()


def test_blocked_slices_behave_like_channels_last_slices():
    buf = _cl(Cs=64)
    a, b = Region.blocked(buf, 0, 32), Region.blocked(buf, 32, 32)
    assert not a.conflicts(b) and a.conflicts(Region.blocked(buf, 16, 32)) and Region.blocked(buf, 16, 32).conflicts(b)
    assert a.rows == 2 and a.hi - a.lo == 2 * 27 * 16 * 2                   # per sample: two blocks of [voxels][16] halves
    widened = Region.blocked(buf, 8, 16)                                   # not 16-aligned: whole blocks, a superset
    assert not widened.exact and widened.conflicts(a) and widened.conflicts(Region.blocked(buf, 16, 16))
    # the same bytes told as two layouts: equal hulls, different strides -> "conflict", never "no conflict"
    assert Region.channels(buf, 0, 32).conflicts(Region.blocked(buf, 32, 32))


def test_equal_hulls_with_different_strides_conflict_and_disjoint_allocations_do_not():
    a = Region.make(1000, 4, 64, 0, 16)
    b = Region.make(1000, 8, 32, 16, 32)             # would be disjoint from a if worked out; not implemented -> conflict
    assert a.conflicts(b) and b.conflicts(a)
    c = Region.make(5000, 4, 64, 0, 16)
    assert not a.conflicts(c) and not c.conflicts(a)
    assert not Region.contiguous(0, 100).conflicts(Region.contiguous(100, 50))
    assert Region.contiguous(0, 101).conflicts(Region.contiguous(100, 50))
    gap = Region.contiguous(1000 + 16, 48)           # a contiguous range that fits between two row intervals
    assert not a.conflicts(gap) and not gap.conflicts(a) and a.conflicts(Region.contiguous(1000 + 16, 49))
    shifted = Region.make(1000 + 64 + 16, 2, 64, 0, 48)                   # same stride, other base
    assert not a.conflicts(shifted) and a.conflicts(Region.make(1000 + 64 + 15, 2, 64, 0, 48))


def test_region_conflicts_agree_with_byte_sets():
    g = torch.Generator().manual_seed(0)
    rnd = lambda n: int(torch.randint(0, n, (1,), generator=g))  # noqa: E731
    for _ in range(400):
        S = 8 + rnd(24)
        regs = []
        for _ in range(2):
            lo = rnd(S - 1)
            regs.append(Region.make(rnd(64), 1 + rnd(4), S, lo, lo + 1 + rnd(S - lo - 1) if S - lo - 1 else lo + 1))
        sets = [{r.base + i * r.stride + k for i in range(r.rows) for k in range(r.lo, r.hi)} for r in regs]
        assert regs[0].conflicts(regs[1]) == bool(sets[0] & sets[1]), regs


# ---- clocks ------------------------------------------------------------------------------------------------------------------------
A, B, Cc = Region.contiguous(0, 64), Region.contiguous(64, 64), Region.contiguous(128, 64)


def _kinds(rep):
    return [(h.kind, h.first.name, h.second.name) for h in rep.unordered]


def test_fork_and_join_through_wait_stream():
    t = [launch("p", MAIN, writes=[A]), wait_stream(SIDE, MAIN), launch("c", SIDE, reads=[A], writes=[B]),
         wait_stream(MAIN, SIDE), launch("d", MAIN, reads=[B], writes=[A])]
    rep = analyse(t)
    assert not rep.unordered and rep.examined == 2 and rep.launches == {MAIN: 2, SIDE: 1} and rep.syncs == 2
    assert _kinds(analyse(t[:1] + t[2:])) == [("RAW", "p", "c")]
    assert _kinds(analyse(t[:3] + t[4:])) == [("RAW", "c", "d")]           # WAR on A is the same pair: one entry per pair


def test_an_event_recorded_twice_the_wait_sees_the_record_before_it():
    t = [launch("w1", SIDE, writes=[A]), record("e", SIDE), wait_event(MAIN, "e"), launch("r1", MAIN, reads=[A]),
         launch("w2", SIDE, writes=[B]), record("e", SIDE), launch("r2", MAIN, reads=[B])]
    assert _kinds(analyse(t)) == [("RAW", "w2", "r2")]                     # the wait preceded the second record
    assert not analyse(t[:6] + [wait_event(MAIN, "e")] + t[6:]).unordered
    # the latest record wins: a wait after the second record sees both launches
    late = [launch("w1", SIDE, writes=[A]), record("e", SIDE), launch("w2", SIDE, writes=[B]), record("e", SIDE),
            wait_event(MAIN, "e"), launch("r", MAIN, reads=[A, B])]
    assert not analyse(late).unordered


def test_a_wait_on_an_event_never_recorded_adds_no_edge():
    t = [launch("w", SIDE, writes=[A]), wait_event(MAIN, "never"), launch("r", MAIN, reads=[A])]
    assert _kinds(analyse(t)) == [("RAW", "w", "r")]


def test_transitivity_over_three_streams():
    t = [launch("a", MAIN, writes=[A]), record("e1", MAIN), wait_event(SIDE, "e1"), launch("b", SIDE, reads=[A], writes=[B]),
         record("e2", SIDE), wait_event(THIRD, "e2"), launch("c", THIRD, reads=[A, B])]
    assert not analyse(t).unordered
    assert _kinds(analyse(t[:2] + t[3:])) == [("RAW", "a", "b"), ("RAW", "a", "c")]


def test_a_host_barrier_orders_everything_and_a_stream_synchronize_only_that_stream():
    t = [launch("a", MAIN, writes=[A]), launch("b", SIDE, writes=[B]), host_barrier(), launch("c", THIRD, reads=[A, B]),
         launch("d", SIDE, reads=[A])]
    assert not analyse(t).unordered
    t[2] = host_barrier(stream=MAIN)                 # what MAIN had issued is visible everywhere; SIDE's launch is not
    assert _kinds(analyse(t)) == [("RAW", "b", "c")]
    assert _kinds(analyse(t[:2] + t[3:])) == [("RAW", "a", "c"), ("RAW", "a", "d"), ("RAW", "b", "c")]
    ev = [launch("a", MAIN, writes=[A]), record("e", MAIN), launch("a2", MAIN, writes=[B]), host_barrier(event="e"),
          launch("c", SIDE, reads=[A]), launch("c2", SIDE, reads=[B])]
    assert _kinds(analyse(ev)) == [("RAW", "a2", "c2")]
    # no implicit order between the default stream and another one
    assert _kinds(analyse([launch("a", 0, writes=[A]), launch("b", SIDE, reads=[A])])) == [("RAW", "a", "b")]


# ---- defects -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["RAW", "WAR", "WAW"])
def test_each_hazard_kind_is_reported_and_gone_with_the_edge(kind):
    first = launch("first", MAIN, reads=[A] if kind == "WAR" else [], writes=[] if kind == "WAR" else [A])
    second = launch("second", SIDE, reads=[A] if kind == "RAW" else [], writes=[] if kind == "RAW" else [A])
    rep = analyse([first, second], so.BufferNames())
    assert len(rep.unordered) == 1
    h = rep.unordered[0]
    assert (h.kind, h.first, h.second, h.first.stream, h.second.stream) == (kind, first, second, MAIN, SIDE)
    names = so.BufferNames()
    names.add("buf", 0, 64)
    assert analyse([first, second], names).unordered[0].buffer == "buf"
    assert not analyse([first, wait_stream(SIDE, MAIN), second]).unordered
    assert not analyse([first, record("e", MAIN), wait_event(SIDE, "e"), second]).unordered
    assert len(analyse([first, wait_stream(MAIN, SIDE), second]).unordered) == 1          # the edge the wrong way round
    assert not analyse([launch("first", MAIN, reads=[A]), launch("second", SIDE, reads=[A])]).unordered   # two reads


def _mini(steps=2):
    """The Swin step in small: a main chain writes hs; ``ready`` forks the side block, which reads xin / hs / cur_add with its own
    scratch and writes the skip half of cat; the main stream writes the other half and reads the whole after the event; the next
    step's step_begin and tail overwrite what the side block read."""
    cat = torch.zeros((1, 2, 2, 2, 16), dtype=torch.float16)
    up, skip = Region.channels(cat, 0, 8), Region.channels(cat, 8, 8)
    base = cat.data_ptr() + 4096
    xin, hs, cur_add, raw1, raw1b, dec = (Region.contiguous(base + 256 * i, 256) for i in range(6))
    t = []
    for s in range(steps):
        t += [launch("step_begin", MAIN, writes=[cur_add], label=f"{s}"),
              launch("swin", MAIN, reads=[xin, cur_add], writes=[hs], label=f"{s}"),
              wait_stream(SIDE, MAIN),
              launch("enc.conv", SIDE, reads=[xin, hs], writes=[raw1b], label=f"{s}"),
              launch("enc.tail", SIDE, reads=[raw1b, cur_add], writes=[skip], label=f"{s}"),
              record("enc_done", SIDE),
              launch("deep", MAIN, reads=[hs], writes=[raw1], label=f"{s}"),
              launch("deconv", MAIN, reads=[raw1], writes=[up], label=f"{s}"),
              wait_event(MAIN, "enc_done"),
              launch("dec.conv", MAIN, reads=[up, skip], writes=[dec], label=f"{s}"),
              launch("tail", MAIN, reads=[dec], writes=[xin], label=f"{s}")]
    names = so.BufferNames()
    for n, r in (("xin", xin), ("hs", hs), ("cur_add", cur_add), ("raw1", raw1), ("raw1b", raw1b), ("dec", dec)):
        names.add(n, r.base, r.hi)
    names.add_tensor("cat", cat)
    return t, names, cat


def _without(trace, kind, nth):
    hits = [i for i, r in enumerate(trace) if isinstance(r, so.Sync) and r.kind == kind]
    return trace[:hits[nth]] + trace[hits[nth] + 1:]


def test_the_swin_miniature_passes_and_fails_where_a_wait_is_deleted():
    t, names, cat = _mini()
    rep = analyse(t, names)
    assert not rep.unordered, [str(h) for h in rep.unordered]
    assert rep.launches == {MAIN: 12, SIDE: 4} and rep.syncs == 6 and rep.examined > 0
    got = lambda tr: {(h.kind, h.first.name + h.first.label, h.second.name + h.second.label, h.buffer)  # noqa: E731
                      for h in analyse(tr, names).unordered}
    # the fork of the first step: the side block reads what the main chain has not been ordered to have written
    assert got(_without(t, "wait_stream", 0)) == {("RAW", "swin0", "enc.conv0", "hs"), ("RAW", "step_begin0", "enc.tail0", "cur_add")}
    # the event wait of the first step: the decoder reads the skip half; the next step's overwrites lose their order too
    assert got(_without(t, "wait_event", 0)) == {("RAW", "enc.tail0", "dec.conv0", "cat"), ("WAR", "enc.conv0", "tail0", "xin"),
                                                 ("WAR", "enc.tail0", "step_begin1", "cur_add"), ("WAR", "enc.conv0", "swin1", "hs")}
    # the fork of the second step: besides its own reads, the side block's scratch and cat half are reused with no order after the
    # main stream's read of the first step's skip
    second = got(_without(t, "wait_stream", 1))
    assert {("RAW", "swin1", "enc.conv1", "hs"), ("RAW", "step_begin1", "enc.tail1", "cur_add"), ("RAW", "tail0", "enc.conv1", "xin"),
            ("WAR", "dec.conv0", "enc.tail1", "cat")} <= second
    # the side block on the main chain's scratch
    lo, hi = next((lo, hi) for lo, hi, n in names.items if n == "raw1")
    raw1, raw1b = Region.contiguous(lo, hi - lo), next(Region.contiguous(lo, hi - lo) for lo, hi, n in names.items if n == "raw1b")
    swap = lambda accs: [raw1 if a.region == raw1b else a.region for a in accs]  # noqa: E731
    renamed = [launch(r.name, r.stream, swap(r.reads), swap(r.writes), r.label) if isinstance(r, so.Launch) else r for r in t]
    assert {("WAW", "enc.conv0", "deep0", "raw1"), ("WAR", "enc.tail0", "deep0", "raw1")} <= got(renamed)


# ---- the recorder without a device -------------------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def dua_fake_launch(self, p, stream):
        self.calls.append(("launch", stream.value or 0))
        return 0

    def dua_fake_bytes(self, n):
        return 16 * n


def _fake(stream=MAIN):
    native = types.SimpleNamespace(_lib=_FakeLib())
    ops = types.ModuleType("fake_ops")
    state = dict(stream=stream)

    def good(x, y, c, off=0, scale=1.0):
        native._lib.dua_fake_bytes(3)
        return native._lib.dua_fake_launch(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(state["stream"]))

    def sloppy(x, extra):
        return native._lib.dua_fake_launch(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(state["stream"]))

    def unwrapped(x):
        return native._lib.dua_fake_launch(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(state["stream"]))

    ops.good, ops.sloppy, ops.unwrapped = good, sloppy, unwrapped
    access = dict(good=dict(x="r", y=so.sl("w", "c", "off")), sloppy=dict(x="r"))
    rec = so.Recorder(ops=ops, native=native, access=access, current_stream=lambda: state["stream"], dispatch=False, syncs=False)
    return ops, native, rec, state


def test_the_recorder_logs_a_wrapped_call_and_restores_the_modules():
    ops, native, rec, state = _fake()
    lib, good = native._lib, ops.good
    x, y = torch.zeros(8), torch.zeros((4, 16))
    with rec:
        assert ops.good is not good and native._lib is not lib
        ops.good(x, y, 8, off=8)
        state["stream"] = SIDE
        ops.good(x, y, 8)
    assert ops.good is good and native._lib is lib and lib.calls == [("launch", MAIN), ("launch", SIDE)]
    a, b = so.launches(rec.trace)
    assert (a.name, a.stream, a.label, b.stream) == ("good", MAIN, "dua_fake_launch", SIDE)
    assert [r.region for r in a.reads] == [Region.of_tensor(x)] and [w.region for w in a.writes] == [Region.channels(y, 8, 8)]
    assert [(h.kind, h.buffer) for h in analyse(rec.trace, so.BufferNames().scan(types.SimpleNamespace(y=y))).unordered] == []
    assert b.writes[0].region == Region.channels(y, 0, 8)


def test_an_unclassified_tensor_argument_raises():
    ops, native, rec, _ = _fake()
    with rec:
        ops.sloppy(torch.zeros(8), 3)                                      # a non-tensor needs no classification
        for extra in (torch.zeros(4), [1, torch.zeros(4)], (torch.zeros(2),)):
            with pytest.raises(so.UnclassifiedArgument, match="extra"):
                ops.sloppy(torch.zeros(8), extra)
    assert len(native._lib.calls) == 1


def test_a_native_launch_outside_a_wrapper_or_on_another_stream_raises():
    ops, native, rec, state = _fake()
    x = torch.zeros(8)
    with rec:
        with pytest.raises(so.UnrecordedLaunch, match="outside a wrapped"):
            ops.unwrapped(x)
        assert native._lib.dua_fake_bytes(2) == 32                          # a call without a stream is not a launch

        def moved(x, y, c, off=0, scale=1.0, inner=ops.good.__wrapped__):
            state["stream"] = SIDE                                         # the launch goes to a stream the wrapper did not see
            return inner(x, y, c)

        rec.ops.good = rec._wrap("good", moved)
        with pytest.raises(so.UnrecordedLaunch, match="recorded 0"):
            ops.good(x, torch.zeros((4, 16)), 8)
    assert native._lib.calls == []
