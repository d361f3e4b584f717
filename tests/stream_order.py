"""Happens-before check of the launch order on more than one stream.  No device code: a recorder that logs what is issued, and an
analyser that decides, without timing, whether every pair of conflicting accesses on different streams is ordered by waits.

Trace.  A list of records in issue order:
  * ``Launch(name, stream, reads, writes, label)``: one kernel launch (or aten op); ``reads`` / ``writes`` are lists of ``Access``
    (region, role = the argument it came from).  Atomic accumulation (the statistics words) is a write.
  * ``Sync(kind, ...)``: ``record(event, stream)``, ``wait_event(stream, event)``, ``wait_stream(stream = waiter, other = waited)``,
    ``host_barrier`` (torch.cuda.synchronize: everything; Stream.synchronize / Event.synchronize: that stream's / event's clock
    reaches every stream -- fewer edges than "everything", which can only produce more reports).
  * ``Note(kind, ...)``: ``mark`` (a label the test puts between phases) and ``liveness`` (an operand of a side-stream launch was /
    was not alive at the join, see Recorder(liveness=...)).

Region.  The bytes a launch touches in one buffer: ``rows`` intervals [lo, hi) at ``base + i * stride``.  That is exact for a
channel slice [off, off + c) of a channels-last buffer with row stride Cs (rows x column interval), for a 16-channel-aligned slice
of a 16-channel-blocked buffer [N][Cs / 16][voxels][16] (one interval per sample), for plain contiguous ranges (one row), and for
a 2-D view with one row stride.  Two regions conflict when they share a byte; where exactness is not implemented (two multi-row
regions of different strides over overlapping hulls, arbitrary torch strides -> the hull) the answer is "conflict".

Analyser.  Vector clocks per stream.  A launch advances its stream's component; ``record`` stores the stream's clock in the event
(the latest record wins, a wait sees the record that preceded it in issue order, a wait on an event never recorded adds no edge);
``wait_event`` / ``wait_stream`` merge.  The implicit synchronisation of ``.item()`` / ``.cpu()`` adds no edge, and no order is
assumed between the default stream and torch's (non-blocking) streams.  The result lists every cross-stream pair of launches with a
write of one meeting a read or write of the other and no happens-before in either direction.

Recorder.  A context manager that logs and calls through: it adds no synchronisation and removes none.
  * every function of ``ACCESS`` is wrapped on the ``ops`` module by attribute; the stream is ``torch.cuda.current_stream()`` at the
    call, reads and writes come from ``ACCESS[name]``.  A tensor-valued argument the table does not classify raises
    ``UnclassifiedArgument``: there is no exemption list.  Scratch the wrapper fetches itself (``workspace=None``; ``ops.zeros``)
    is taken from the helpers' return values, a ``workspace=`` callable (the plan's own scratch) is wrapped for the call.
  * ``_native._lib`` is replaced by a proxy that forwards every call and asserts that each ``dua_*`` call that takes a stream
    happens inside a wrapped function, with the stream handle that was recorded: an unrecorded native launch fails.
  * Stream.wait_stream / wait_event / record_event / synchronize, Event.record / wait / synchronize and torch.cuda.synchronize log,
    then call through.
  * on the thread that entered the recorder a TorchDispatchMode records each aten op that touches a device tensor and is not a pure
    view or an allocation (writes: the schema's ``alias_info.is_write`` arguments plus outputs; regions from pointer, sizes and strides).
    Autograd's worker thread is outside the mode; the wrappers and the proxy are thread-safe and do see it.
"""
import ctypes
import inspect
import threading
import weakref
from dataclasses import dataclass, field

import torch


# ---- regions ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Region:
    base: int
    rows: int
    stride: int
    lo: int
    hi: int
    exact: bool = True

    @staticmethod
    def contiguous(ptr, nbytes, exact=True):
        return Region(int(ptr), 1, 0, 0, int(nbytes), exact)

    @staticmethod
    def make(base, rows, stride, lo, hi, exact=True):
        """rows intervals [lo, hi) at base + i * stride; whole rows (or one row) collapse to a contiguous range."""
        assert rows >= 1 and 0 <= lo < hi
        if rows == 1 or (lo == 0 and hi == stride):
            return Region(base + lo, 1, 0, 0, (rows - 1) * stride + hi - lo, exact)
        assert hi <= stride, "a row interval reaches into the next row"
        return Region(int(base + lo), int(rows), int(stride), 0, int(hi - lo), exact)        # canonical: lo = 0

    @staticmethod
    def of_tensor(t):
        """What a tensor covers: exact when it is contiguous or has unit stride along its last dimension and one row stride,
        else the hull of its elements (a superset)."""
        es = t.element_size()
        if t.numel() == 0:
            return None
        if t.is_contiguous():
            return Region.contiguous(t.data_ptr(), t.numel() * es)
        dims = [(s, st) for s, st in zip(t.shape, t.stride()) if s > 1]
        if dims and dims[-1][1] == 1 and all(st > 0 for _, st in dims):
            inner, outer = dims[-1][0], dims[:-1]
            uniform = all(outer[i][1] == outer[i + 1][1] * outer[i + 1][0] for i in range(len(outer) - 1))
            if outer and uniform and outer[-1][1] >= inner:
                rows = 1
                for s, _ in outer:
                    rows *= s
                return Region.make(t.data_ptr(), rows, outer[-1][1] * es, 0, inner * es)
        extent = 1 + sum((s - 1) * abs(st) for s, st in dims)
        lowest = sum((s - 1) * st for s, st in dims if st < 0)
        return Region.contiguous(t.data_ptr() + lowest * es, extent * es, exact=False)

    @staticmethod
    def channels(t, off, c):
        """Channels [off, off + c) of a channels-last tensor [..., Cs] (contiguous, or itself a channel slice of one)."""
        es, Cs = t.element_size(), t.shape[-1]
        assert 0 <= off and c > 0 and off + c <= Cs, (off, c, Cs)
        whole = Region.of_tensor(t)
        rows = t.numel() // Cs
        if whole.rows == 1 and whole.exact and whole.hi == rows * Cs * es:          # contiguous
            return Region.make(whole.base, rows, Cs * es, off * es, (off + c) * es)
        if whole.exact and whole.rows == rows and whole.hi - whole.lo == Cs * es:   # a channel slice already
            return Region.make(whole.base, rows, whole.stride, whole.lo + off * es, whole.lo + (off + c) * es)
        return Region(whole.base, 1, 0, 0, whole.hi, False)

    @staticmethod
    def blocked(t, off, c):
        """Channels [off, off + c) of a 16-channel-blocked buffer [N][Cs / 16][voxels][16] carrying the channels-last shape
        [N, D, H, W, Cs]; a slice that is not 16-aligned is widened to whole blocks."""
        es, N, Cs = t.element_size(), t.shape[0], t.shape[-1]
        assert t.is_contiguous() and Cs % 16 == 0 and 0 <= off and c > 0 and off + c <= Cs
        vox = t.numel() // (N * Cs)
        b0, b1 = off // 16, -(-(off + c) // 16)
        return Region.make(t.data_ptr(), N, Cs * vox * es, b0 * vox * 16 * es, b1 * vox * 16 * es, exact=(off % 16 == 0 and c % 16 == 0))

    def hull(self):
        return self.base + self.lo, self.base + (self.rows - 1) * self.stride + self.hi

    def conflicts(self, other):
        a0, a1 = self.hull()
        b0, b1 = other.hull()
        if a1 <= b0 or b1 <= a0:
            return False
        if self.rows > 1 and other.rows > 1 and self.stride != other.stride:
            return True                                  # not implemented exactly: never "no conflict"
        S = self.stride if self.rows > 1 else other.stride
        if S == 0:
            return True                                  # two intervals whose hulls overlap
        w1, w2 = self.hi - self.lo, other.hi - other.lo
        delta = b0 - a0
        # rows i of self and j of other share a byte iff -w2 < delta + (j - i) S < w1
        k_min = max(-(self.rows - 1), (-w2 - delta) // S + 1)
        k_max = min(other.rows - 1, -((delta - w1) // S) - 1)
        return k_min <= k_max


# ---- trace -----------------------------------------------------------------------------------------------------------------------
@dataclass
class Access:
    region: Region
    role: str


@dataclass
class Launch:
    name: str
    stream: int
    reads: list = field(default_factory=list)
    writes: list = field(default_factory=list)
    label: str = ""
    depth: int = 0
    kind: str = "launch"


@dataclass
class Sync:
    kind: str                    # record | wait_event | wait_stream | host_barrier
    stream: int = None           # record: the recording stream; wait_*: the waiter; host_barrier: the stream synchronised or None
    event: int = None
    other: int = None            # wait_stream: the stream waited for


@dataclass
class Note:
    kind: str
    label: str = ""
    data: dict = field(default_factory=dict)


def launch(name, stream, reads=(), writes=(), label=""):
    """A synthetic launch; reads / writes: Regions (or Accesses)."""
    acc = lambda rs: [r if isinstance(r, Access) else Access(r, "") for r in rs]  # noqa: E731
    return Launch(name, stream, acc(reads), acc(writes), label)


def record(event, stream):
    return Sync("record", stream=stream, event=event)


def wait_event(stream, event):
    return Sync("wait_event", stream=stream, event=event)


def wait_stream(waiter, waited):
    return Sync("wait_stream", stream=waiter, other=waited)


def host_barrier(stream=None, event=None):
    return Sync("host_barrier", stream=stream, event=event)


class BufferNames:
    """pointer -> name of the smallest named allocation that contains it."""

    def __init__(self):
        self.items = []

    def add(self, name, ptr, nbytes):
        if nbytes > 0:
            self.items.append((int(ptr), int(ptr) + int(nbytes), name))

    def add_tensor(self, name, t):
        if isinstance(t, torch.Tensor) and t.numel():
            r = Region.of_tensor(t)
            self.items.append((*r.hull(), name))

    def scan(self, obj, prefix=""):
        """Every tensor attribute of ``obj``, and tensors in its list / tuple / dict attributes one level down."""
        for k, v in vars(obj).items():
            if isinstance(v, torch.Tensor):
                self.add_tensor(prefix + k, v)
            elif isinstance(v, (list, tuple)):
                for i, e in enumerate(v):
                    self.add_tensor(f"{prefix}{k}[{i}]", e)
            elif isinstance(v, dict):
                for i, e in v.items():
                    self.add_tensor(f"{prefix}{k}[{i}]", e)
        return self

    def name(self, ptr):
        best = None
        for lo, hi, n in self.items:
            if lo <= ptr < hi and (best is None or hi - lo < best[0]):
                best = (hi - lo, n)
        return best[1] if best else f"?{ptr:x}"

    def of(self, region):
        return self.name(region.hull()[0])


# ---- analysis --------------------------------------------------------------------------------------------------------------------
@dataclass
class Hazard:
    kind: str                    # RAW | WAR | WAW, by issue order
    first: Launch
    second: Launch
    buffer: str
    i: int
    j: int

    def __str__(self):
        f = lambda l: f"{l.name}{'(' + l.label + ')' if l.label else ''}@{l.stream:x}"  # noqa: E731
        return f"{self.kind} on {self.buffer}: {f(self.first)} [{self.i}] || {f(self.second)} [{self.j}]"


@dataclass
class Report:
    unordered: list
    examined: int                # cross-stream conflicting pairs
    launches: dict               # stream -> count
    syncs: int
    clocks: dict                 # stream -> its vector clock at the end of the trace
    ticks: list                  # per trace index: (stream, tick, clock) of a launch, else None

    def ordered(self, i, j):
        """launch at trace index i happens before the launch at trace index j"""
        (si, ti, _), (sj, _, cj) = self.ticks[i], self.ticks[j]
        return (i < j) if si == sj else (i < j and cj.get(si, 0) >= ti)

    def summary(self):
        per = ", ".join(f"{s:x}: {n}" for s, n in sorted(self.launches.items()))
        return f"launches per stream {{{per}}}, {self.syncs} sync records, {self.examined} cross-stream conflicting pairs, " \
               f"{len(self.unordered)} unordered"


def _merge(into, other):
    for s, t in other.items():
        if into.get(s, 0) < t:
            into[s] = t


def _first_conflict(xs, ys):
    for a in xs:
        for b in ys:
            if a.region.conflicts(b.region):
                return a
    return None


def analyse(trace, names=None):
    names = names or BufferNames()
    clocks, events, floor = {}, {}, {}
    ticks, launches, nsync = [None] * len(trace), {}, 0

    def clock(s):
        if s not in clocks:
            clocks[s] = dict(floor)
        return clocks[s]

    for idx, r in enumerate(trace):
        if isinstance(r, Launch):
            c = clock(r.stream)
            c[r.stream] = c.get(r.stream, 0) + 1
            ticks[idx] = (r.stream, c[r.stream], dict(c))
            launches[r.stream] = launches.get(r.stream, 0) + 1
        elif isinstance(r, Sync):
            nsync += 1
            if r.kind == "record":
                events[r.event] = dict(clock(r.stream))
            elif r.kind == "wait_event":
                if r.event in events:
                    _merge(clock(r.stream), events[r.event])
            elif r.kind == "wait_stream":
                _merge(clock(r.stream), clock(r.other))
            elif r.kind == "host_barrier":
                if r.event is not None:
                    src = dict(events.get(r.event, {}))
                elif r.stream is not None:
                    src = dict(clock(r.stream))
                else:
                    src = {}
                    for c in clocks.values():
                        _merge(src, c)
                _merge(floor, src)
                for c in clocks.values():
                    _merge(c, src)
            else:
                raise ValueError(r.kind)
    rep = Report([], 0, launches, nsync, {s: dict(c) for s, c in clocks.items()}, ticks)
    idxs = [i for i, r in enumerate(trace) if isinstance(r, Launch) and (r.reads or r.writes)]
    hulls = {}
    for i in idxs:
        hs = [a.region.hull() for a in trace[i].reads + trace[i].writes]
        hulls[i] = (min(h[0] for h in hs), max(h[1] for h in hs))
    for n, i in enumerate(idxs):
        a = trace[i]
        for j in idxs[n + 1:]:
            b = trace[j]
            if a.stream == b.stream or hulls[i][1] <= hulls[j][0] or hulls[j][1] <= hulls[i][0]:
                continue
            hit = None
            for kind, xs, ys in (("RAW", a.writes, b.reads), ("WAW", a.writes, b.writes), ("WAR", a.reads, b.writes)):
                acc = _first_conflict(xs, ys) if xs and ys else None
                if acc is not None:
                    hit = (kind, acc)
                    break
            if hit is None:
                continue
            rep.examined += 1
            if not rep.ordered(i, j):
                rep.unordered.append(Hazard(hit[0], a, b, names.of(hit[1].region), i, j))
    return rep


# ---- the access table ---------------------------------------------------------------------------------------------------------------
class UnclassifiedArgument(AssertionError):
    pass


class UnrecordedLaunch(AssertionError):
    pass


def sl(mode, c, off=0, blocked=None):
    """channel slice [off, off + c) of the argument; c / off: an argument's name, a number or a function of the bound arguments;
    ``blocked``: the name of the flag that says the buffer is 16-channel-blocked."""
    return ("slice", mode, c, off, blocked)


def _maybe_rw(flag):
    return lambda a: "rw" if a.get(flag) is not None else "r"


NORM, WS = "norm", "ws"
_CONV_IN = dict(w_packed="r", bias_pad="r")
ACCESS = {
    # layout moves
    "to_channels_last": dict(src="r", dst=sl("w", lambda a: max(a["src"].shape[1], a["c_fill"] or 0), "c_off")),
    "to_channels_last_rows": dict(parts="r", dst="w"),
    "from_channels_last": dict(src=sl("r", "C_", "c_off"), out="w", ret="w"),
    # weight packing
    "pack_conv3_weights": dict(w="r", bias="r", ret="w"),
    "pack_conv3_weights_dgrad": dict(w="r", ret=("w", None)),           # (packed, the shared never-written zero bias)
    "pack_deconv_weights": dict(w="r", bias="r", ret="w"),
    "pack_upconv_weights": dict(wc="r", bc="r", wd="r", bd="r", ret="w"),
    "ConvPacks.run": dict(self=lambda a: [(w, "r") for w, *_ in a["self"].items],
                          ret=lambda ret: [(v, "w") for v in ret.out.values() if v is not None]),
    # convolutions
    "conv3d_k3": dict(x=sl("r", "cin", "cin_off", "in_blocked"), y=sl("w", "cout", "cout_off", "out_blocked"), out_stats="rw",
                      norm=NORM, workspace=WS, **_CONV_IN),
    "conv3d_k3_wgrad": dict(x=sl("r", "cin", "cin_off"), dy=sl("r", "cout", "cout_off"), dw="rw", perm="r", workspace=WS),
    "conv3d_k3_dgrad_reduce": dict(dy=sl("r", "cin"), dx=sl("w", "cout"), raw=sl("r", "cout"), norm=NORM, sums="rw", **_CONV_IN),
    "deconv_k2s2": dict(x=sl("r", "cin", "cin_off"), y=sl("w", "cout", "cout_off", "out_blocked"), norm=NORM, **_CONV_IN),
    "deconv_k2s2_bwd": dict(x=sl("r", "cin", "cin_off"), dy=sl("r", "cout", "cout_off"), w="r", ret="w"),
    "deconv_res": dict(lo=sl("r", "cin", "cin_off"), w_packed="r", xs=sl("r", "cs", "cs_off"), ws_packed="r",
                       y=sl("w", "cout", "cout_off"), stats="rw"),
    "upconv_k3": dict(xs=sl("r", "cskip", "cskip_off", "in_blocked"), u=sl("r", "cu", "cu_off"), norm=NORM, w_skip="r", wu="r", btab="r",
                      y=sl("w", "cout", "cout_off", "out_blocked"), out_stats="rw"),
    # normalisation, pooling, head, loss
    "instnorm_finalize": dict(norm=NORM, ret="w"),
    "instnorm_stats": dict(x=sl("r", "Cc", "c_off"), stats="rw"),
    "stats_channel_sums": dict(stats="r", ret="w"),
    "instnorm_bwd": dict(dA=sl("r", "Cc", "da_off"), raw=sl("r", "Cc"), norm=NORM, dY=sl("w", "Cc", "dy_off"), dadd_out="w", sums="rw",
                         ret="w"),
    "maxpool2_bwd_add": dict(act=sl("r", "Cc", "act_off"), dA=sl("r", "Cc", "da_off"), dP=sl("r", "Cc"), ret="w"),
    "materialize": dict(raw=sl("r", "Cc"), norm=NORM, out=sl("w", "Cc", "out_off", "out_blocked"), emb=sl("r", "Cc"), pooled=sl("w", "Cc")),
    "head_fwd": dict(u="r", weight="r", bias="r", out="w", ret="w"),
    "head_bwd": dict(dlogits="r", u="r", weight="r", ret="w"),
    "seg_loss_reduce": dict(logits="r", labels="r", ret="w"),
    "seg_loss_finish": dict(sums="r", out="w", mn="r"),
    "multi_neighbor_partials": dict(logits="r", labels="r", ret="w"),
    "seg_loss_grad": dict(logits="r", labels="r", sums="r", gscale="r", ret="w"),
    # training glue
    "q_sample": dict(x0="r", eps="r", coef="r", out="w", ret="w"),
    "q_sample_affine": dict(src="r", a="r", b="r", eps="r", sched="r", t="r", out="w", ret="w"),
    "temb_train_fwd": dict(t="r", w0="r", b0="r", w1="r", b1="r", proj_w="r", proj_b="r", ret="w"),
    "temb_train_bwd": dict(dadd="r", saved="r", w1="r", proj_w="r", ret="w"),
    "grads_nonfinite": dict(grads="r", found_inf="rw"),
    "adamw_step": dict(params="rw", grads="rw", ms="rw", vs="rw", step="r", lr_dev="r", grad_scale="r", found_inf="r"),
    "adamw_advance": dict(step="rw", found_inf="rw", scale="rw", growth="rw", seen="rw"),
    # sampler
    "temb_table": dict(timesteps="r", freqs="r", w0="r", b0="r", w1="r", b1="r", w_cat="r", b_cat="r", out="w", ret="w"),
    "step_begin": dict(table="r", cur_add="w", rows_per_sample="r", row_of_step="r", counter="rw", coef_table="r", cur_coef="w",
                       step_word="w", err_word="rw", clear="w"),
    "final_conv_sampler": dict(raw=sl("r", lambda a: min(a["K"], a["raw"].shape[-1])), norm=NORM, wf="r", bf="r", coef="r", x_state="rw",
                               noise="r", step_word="r", xin=sl("w", "num_classes"), xstart_sum="rw", logits="w", xstart="w",
                               seed_dev="r",
                               residual=lambda a: [] if a["residual"] is None else [
                                   (a["residual"][0], sl("r", a["residual"][4])), (a["residual"][1], NORM),
                                   (a["residual"][2], sl("r", a["residual"][4], a["residual"][3]))]),
    "denoiser_step": dict(plan_struct="struct"),
    "suf_accumulate": dict(logits="r", acc="rw", step_coef="r", step_word="r", err_word="rw"),
    # Swin
    "window_attention": dict(qkv="r", bias_t="r", mask_t="r", region_ids="r", out="w", bias_table="r", ret="w"),
    "patch_merge_norm": dict(x="r", gamma="r", beta="r", y="r", out="w", ret="w"),
    "residual_norm_act": dict(raw="r", norm=NORM, res=sl("r", lambda a: a["raw"].shape[-1], "res_off"), res_norm=NORM,
                              out=sl("w", lambda a: a["raw"].shape[-1], "out_off"),
                              post_add=sl("r", lambda a: a["raw"].shape[-1], "post_off"),
                              ra_src=sl("r", lambda a: a["raw"].shape[-1], "ra_off"), ret="w"),
    "window_gather_norm": dict(x=_maybe_rw("y"), gamma="r", beta="r", out="w", y="r"),
    "window_scatter_add_norm": dict(x="rw", yw="r", gamma="r", beta="r", out="w"),
    "stage_out": dict(y="r", out=sl("w", "Cc", "out_off"), tadd="r", emb="r", x="w"),
    "patch_embed": dict(xin=sl("r", "cin_packed"), w_packed="r", bias="r", out=sl("w", lambda a: a["w_packed"].shape[-1], "out_off"),
                        tadd="r", emb="r", x="w"),
    "gelu_": dict(x="rw"),
    "token_linear": dict(A="r", W="r", bias="r", out=sl("w", lambda a: a["W"].shape[0], "out_off"), x="rw", stats="rw", gamma="r",
                         beta="r", ln_out="w"),
    "token_gemm": dict(A="r", W="r", bias="r", out=sl("w", lambda a: a["W"].shape[0], "out_off"), x="rw", workspace=WS),
    "swin_mlp": dict(ln2="r", w1="r", b1="r", w2="r", b2="r", x="rw"),
    "linear_f32": dict(x="r", w="r", bias="r", out="w", ret="w"),
}
# helpers whose return value is scratch of the launch that called them
HELPERS = ("_wgrad_ws", "splitk_ws", "_gemm_ws", "zeros", "stats_buffer", "instnorm_bwd_sums")
# aten ops that allocate without launching
_NO_LAUNCH = ("aten::empty", "aten::new_empty", "aten::empty_like", "aten::empty_strided", "aten::new_empty_strided",
              "aten::resize_", "aten::set_", "aten::record_stream")


def _holds_tensor(v):
    if isinstance(v, torch.Tensor):
        return True
    if isinstance(v, (list, tuple)):
        return any(_holds_tensor(e) for e in v)
    if isinstance(v, dict):
        return any(_holds_tensor(e) for e in v.values())
    return hasattr(v, "keep") and hasattr(v, "ref")          # ops.Norm


def _tensors(v):
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, (list, tuple)):
        for e in v:
            yield from _tensors(e)
    elif isinstance(v, dict):
        for e in v.values():
            yield from _tensors(e)


_PLAN_STRUCT = (("temb_table", "r", None), ("rows_per_sample", "r", None), ("row_of_step", "r", None), ("coef_table", "r", None),
                ("counter", "rw", None), ("cur_add", "rw", None), ("cur_coef", "rw", None), ("step_word", "rw", None),
                ("err_word", "rw", None), ("stat_arena", "rw", "stat_bytes"), ("workspace", "rw", "workspace_bytes"),
                ("tail_raw", "r", None), ("wf", "r", None), ("bf", "r", None), ("x_state", "rw", None), ("noise", "r", None),
                ("xin", "rw", None), ("xstart_sum", "rw", None), ("logits", "w", None), ("xstart", "w", None))


class _Frame:
    def __init__(self, launch, handle, tensors):
        self.launch, self.handle, self.arg_ptrs = launch, handle, tensors


class Recorder:
    """``with Recorder(ops, native, names=...) as rec: ...`` -> ``rec.trace``.

    ``ops`` / ``native``: the modules to patch (default: diff_unet_amos_amd.ops / ._native; the host tests pass fakes);
    ``current_stream``: () -> stream handle (default: torch.cuda.current_stream().cuda_stream); ``names``: BufferNames, used by the
    struct argument of denoiser_step to resolve pointers to whole buffers; ``liveness``: names of launches whose operand tensor
    objects are weakly referenced until the next wait_stream on their stream, where a ``liveness`` note says which were alive
    (``alive``) and, with ``owners`` (() -> tensors alive at that moment), whether one of those covers the operand's bytes (``owned``);
    ``dispatch`` / ``syncs``: record aten ops / patch the torch synchronisation methods."""

    def __init__(self, ops=None, native=None, access=None, names=None, current_stream=None, liveness=(), owners=None, dispatch=True,
                 syncs=True):
        if ops is None:
            from diff_unet_amos_amd import ops
        if native is None:
            from diff_unet_amos_amd import _native as native
        self.ops, self.native, self.access = ops, native, ACCESS if access is None else access
        self.names = names or BufferNames()
        self.current_stream = current_stream or (lambda: torch.cuda.current_stream().cuda_stream)
        self.liveness, self.owners, self.dispatch, self.syncs = set(liveness), owners, dispatch, syncs
        self.trace, self.lock, self.tls = [], threading.RLock(), threading.local()
        self.pending, self.keep_events, self._undo, self._mode = {}, [], [], None

    # ---- logging ---------------------------------------------------------------------------------------------------------------
    def _append(self, r):
        with self.lock:
            self.trace.append(r)
        return r

    def mark(self, label):
        self._append(Note("mark", label))

    def _stack(self):
        if not hasattr(self.tls, "stack"):
            self.tls.stack, self.tls.sync_depth = [], 0
        return self.tls.stack

    # ---- accesses ----------------------------------------------------------------------------------------------------------------
    def _value(self, v, args):
        return args[v] if isinstance(v, str) else v(args) if callable(v) else v

    def _apply(self, L, role, value, spec, args):
        """add the accesses of one classified argument"""
        if value is None:
            return
        if callable(spec) and not isinstance(spec, str):
            spec = spec(args)
            if isinstance(spec, list):                    # [(value, spec), ...]
                for v, s in spec:
                    self._apply(L, role, v, s, args)
                return
        if spec == NORM:
            for t in value.keep:
                self._apply(L, role, t, "r", args)
            return
        if spec == WS:
            if isinstance(value, torch.Tensor):
                self._apply(L, role, value, "rw", args)
            return                                         # a callable is wrapped by the caller; None comes through the helpers
        if spec == "struct":
            for fname, mode, size in _PLAN_STRUCT:
                p = getattr(value, fname)
                if p:
                    if size is not None:
                        reg = Region.contiguous(p, getattr(value, size))
                    else:
                        hit = [(lo, hi) for lo, hi, _ in self.names.items if lo <= p < hi]
                        lo, hi = min(hit, key=lambda h: h[1] - h[0]) if hit else (p, p + 1)
                        reg = Region.contiguous(p, hi - p, exact=False)
                    self._add(L, mode, reg, f"{role}.{fname}")
            return
        if isinstance(spec, tuple) and spec and spec[0] == "slice":
            _, mode, c, off, blocked = spec
            c, off = int(self._value(c, args)), int(self._value(off, args) or 0)
            reg = (Region.blocked if (blocked and args.get(blocked)) else Region.channels)(value, off, c)
            self._add(L, mode, reg, role)
            return
        if isinstance(spec, tuple):                       # per element of a returned tuple
            for v, s in zip(value, spec):
                if s is not None:
                    self._apply(L, role, v, s, args)
            return
        assert spec in ("r", "w", "rw"), spec
        for t in _tensors(value):
            self._add(L, spec, Region.of_tensor(t), role)

    def _add(self, L, mode, region, role):
        if region is None:
            return
        if "r" in mode:
            L.reads.append(Access(region, role))
        if "w" in mode:
            L.writes.append(Access(region, role))

    # ---- ops wrappers --------------------------------------------------------------------------------------------------------------
    def _wrap(self, name, fn):
        spec = self.access[name]
        sig = inspect.signature(fn)
        rec = self

        def wrapper(*a, **kw):
            if getattr(rec.ops, "_RECORD", None) is not None:       # engine.Plan writing its op list: nothing is launched
                return fn(*a, **kw)
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            args = dict(bound.arguments)
            handle = rec.current_stream()
            stack = rec._stack()
            L = Launch(name, handle, depth=len(stack))
            for k, v in args.items():
                if k in spec:
                    rec._apply(L, k, v, spec[k], args)
                elif _holds_tensor(v):
                    raise UnclassifiedArgument(f"ops.{name}: tensor-valued argument {k!r} is not classified in ACCESS")
            for k, v in args.items():                               # a plan's own scratch: nbytes -> tensor
                if spec.get(k) == WS and callable(v) and not isinstance(v, torch.Tensor):
                    def owned(nbytes, _v=v, _k=k):
                        t = _v(nbytes)
                        rec._apply(L, _k, t, "rw", {})
                        return t
                    bound.arguments[k] = owned
            frame = _Frame(L, handle, {t.data_ptr() for v in args.values() for t in _tensors(getattr(v, "keep", v))})
            rec._append(L)
            if name in rec.liveness:
                refs = [(k, weakref.ref(v), Region.of_tensor(v)) for k, v in args.items() if isinstance(v, torch.Tensor)]
                with rec.lock:
                    rec.pending.setdefault(handle, []).append((L, refs))
            stack.append(frame)
            try:
                ret = fn(*bound.args, **bound.kwargs)
            finally:
                stack.pop()
            if "ret" in spec and ret is not None:
                rs = spec["ret"]
                if callable(rs):
                    for v, s in rs(ret):
                        rec._apply(L, "return", v, s, {})
                elif isinstance(rs, tuple):
                    rec._apply(L, "return", ret, rs, {})
                else:
                    for t in _tensors(ret):
                        if t.data_ptr() not in frame.arg_ptrs:        # an argument handed back was classified as an argument
                            rec._apply(L, "return", t, rs, {})
            return ret

        wrapper.__wrapped__ = fn
        return wrapper

    def _helper(self, name, fn):
        rec = self

        def wrapper(*a, **kw):
            t = fn(*a, **kw)
            stack = rec._stack()
            if stack and isinstance(t, torch.Tensor):
                rec._apply(stack[-1].launch, name, t, "rw", {})
            return t

        return wrapper

    # ---- native proxy ----------------------------------------------------------------------------------------------------------------
    class _Proxy:
        def __init__(self, rec, lib):
            object.__setattr__(self, "_rec", rec)
            object.__setattr__(self, "_lib", lib)

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith("dua_"):
                return fn
            rec = self._rec

            def call(*args):
                if args and isinstance(args[-1], ctypes.c_void_p):      # the trailing stream of a launching entry point
                    handle = args[-1].value or 0
                    stack = rec._stack()
                    if not stack:
                        raise UnrecordedLaunch(f"{name}: native launch outside a wrapped ops function")
                    if handle != stack[-1].handle:
                        raise UnrecordedLaunch(f"{name}: launched on stream {handle:x}, recorded {stack[-1].handle:x}")
                    stack[0].launch.label = stack[0].launch.label or name
                return fn(*args)

            return call

    # ---- torch synchronisation -----------------------------------------------------------------------------------------------------
    def _patch(self, owner, attr, new):
        old = getattr(owner, attr)
        self._undo.append((owner, attr, old))
        setattr(owner, attr, new(old))

    def _outer(self):
        self._stack()
        return self.tls.sync_depth == 0

    def _sync_call(self, old, log_before, log_after, *a, **kw):
        outer = self._outer()
        if outer and log_before:
            log_before()
        self.tls.sync_depth += 1
        try:
            ret = old(*a, **kw)
        finally:
            self.tls.sync_depth -= 1
        if outer and log_after:
            log_after(ret)
        return ret

    def _event(self, e):
        self.keep_events.append(e)                       # keeps id(e) from being reused
        return id(e)

    def _join(self, waiter, waited):
        self._append(wait_stream(waiter, waited))
        with self.lock:
            pend = self.pending.pop(waited, [])
        owned = [Region.of_tensor(t).hull() for t in (self.owners() if pend and self.owners else []) if t is not None and t.numel()]
        for L, refs in pend:
            for role, ref, reg in refs:
                lo, hi = reg.hull()
                self._append(Note("liveness", L.name, dict(launch=L, role=role, alive=ref() is not None, stream=waited,
                                                           owned=any(a <= lo and hi <= b for a, b in owned))))

    def _patch_syncs(self):
        S, E, rec = torch.cuda.Stream, torch.cuda.Event, self
        cur = self.current_stream
        self._patch(S, "wait_stream", lambda old: lambda s, other: rec._sync_call(
            old, lambda: rec._join(s.cuda_stream, other.cuda_stream), None, s, other))
        self._patch(S, "wait_event", lambda old: lambda s, e: rec._sync_call(
            old, lambda: rec._append(wait_event(s.cuda_stream, rec._event(e))), None, s, e))
        self._patch(S, "record_event", lambda old: lambda s, e=None: rec._sync_call(
            old, None, lambda ret: rec._append(record(rec._event(ret), s.cuda_stream)), s, e))
        self._patch(S, "synchronize", lambda old: lambda s: rec._sync_call(
            old, None, lambda ret: rec._append(host_barrier(stream=s.cuda_stream)), s))
        self._patch(E, "record", lambda old: lambda e, stream=None: rec._sync_call(
            old, lambda: rec._append(record(rec._event(e), stream.cuda_stream if stream is not None else cur())), None, e, stream))
        self._patch(E, "wait", lambda old: lambda e, stream=None: rec._sync_call(
            old, lambda: rec._append(wait_event(stream.cuda_stream if stream is not None else cur(), rec._event(e))), None, e, stream))
        self._patch(E, "synchronize", lambda old: lambda e: rec._sync_call(
            old, None, lambda ret: rec._append(host_barrier(event=rec._event(e))), e))
        self._patch(torch.cuda, "synchronize", lambda old: lambda device=None: rec._sync_call(
            old, None, lambda ret: rec._append(host_barrier()), device))

    # ---- aten ops --------------------------------------------------------------------------------------------------------------------
    def _dispatch_mode(self):
        from torch.utils._python_dispatch import TorchDispatchMode
        rec = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                kwargs = kwargs or {}
                out = func(*args, **kwargs)
                rec._aten(func, args, kwargs, out)
                return out

        return Mode()

    def _aten(self, func, args, kwargs, out):
        schema = func._schema
        if schema.name.startswith(_NO_LAUNCH):
            return
        rets = schema.returns
        writes_arg = any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments)
        if rets and not writes_arg and all(r.alias_info is not None for r in rets):
            return                                                   # a pure view
        L = Launch(schema.name, None, kind="aten", depth=len(self._stack()))
        pos = [a for a in schema.arguments if not a.kwarg_only]
        byname = {a.name: a for a in schema.arguments}
        seen = set()
        for i, v in list(enumerate(args)) + list(kwargs.items()):
            a = (pos[i] if i < len(pos) else None) if isinstance(i, int) else byname.get(i)
            wr = a is not None and a.alias_info is not None and a.alias_info.is_write
            for t in _tensors(v):
                if t.is_cuda and t.numel():
                    seen.add(t.data_ptr())
                    self._add(L, "rw" if wr else "r", Region.of_tensor(t), a.name if a is not None else "arg")
        for t in _tensors(out):
            if t.is_cuda and t.numel() and t.data_ptr() not in seen:
                self._add(L, "w", Region.of_tensor(t), "out")
        if L.reads or L.writes:
            L.stream = self.current_stream()
            self._append(L)

    # ---- context ---------------------------------------------------------------------------------------------------------------------
    def __enter__(self):
        lib = self.native.lib() if hasattr(self.native, "lib") else self.native._lib
        self._patch(self.native, "_lib", lambda old: Recorder._Proxy(self, lib))
        for name in self.access:
            owner, attr = self.ops, name
            if "." in name:
                cls, attr = name.split(".")
                owner = getattr(self.ops, cls, None)
            if owner is not None and hasattr(owner, attr):
                self._patch(owner, attr, lambda old, name=name: self._wrap(name, old))
        for name in HELPERS:
            if hasattr(self.ops, name):
                self._patch(self.ops, name, lambda old, name=name: self._helper(name, old))
        if self.syncs:
            self._patch_syncs()
        if self.dispatch:
            self._mode = self._dispatch_mode()
            self._mode.__enter__()
        return self

    def __exit__(self, *exc):
        if self._mode is not None:
            self._mode.__exit__(*exc)
            self._mode = None
        for owner, attr, old in reversed(self._undo):
            setattr(owner, attr, old)
        self._undo = []
        return False


# ---- trace helpers ---------------------------------------------------------------------------------------------------------------
def launches(trace, top=True):
    return [r for r in trace if isinstance(r, Launch) and (r.depth == 0 or not top)]


def syncs(trace):
    return [r for r in trace if isinstance(r, Sync)]


def between(trace, begin, end):
    """the records between the marks ``begin`` and ``end``"""
    i = next(k for k, r in enumerate(trace) if isinstance(r, Note) and r.kind == "mark" and r.label == begin)
    j = next(k for k, r in enumerate(trace) if isinstance(r, Note) and r.kind == "mark" and r.label == end)
    return trace[i + 1:j]


def shape_of(trace):
    """The trace with streams and events renamed by order of first appearance: what two passes of the same program share when
    they run on different streams (an eager pass and a capture pass)."""
    smap, emap, out = {}, {}, []
    s = lambda h: None if h is None else smap.setdefault(h, f"s{len(smap)}")  # noqa: E731
    e = lambda h: None if h is None else emap.setdefault(h, f"e{len(emap)}")  # noqa: E731
    for r in trace:
        if isinstance(r, Launch):
            out.append(("launch", r.name, r.label, s(r.stream), r.depth))
        elif isinstance(r, Sync):
            out.append((r.kind, s(r.stream), e(r.event), s(r.other)))
    return out
