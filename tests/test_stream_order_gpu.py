"""The shipped launch sequences that use (or must not use) a second stream, recorded once and held to the happens-before analysis of
tests/stream_order.py: every pair of conflicting accesses on different streams must be ordered by a chain of waits.  Nothing here
depends on timing, nothing removes or delays a synchronisation in what executes (defects are planted in recorded traces), no captured
graph is replayed.

  * SwinPlan (swin_engine.py): run_encoder, two consecutive sampler steps and one denoise of the three cases of swin_plan_cases, with
    ``two_streams`` at its default; the order knobs (conv3_first, side_plan, two_streams = False); the warm-up and capture passes of
    capture_step against the eager step; three planted defects.
  * engine.Plan (DiffUNet): single-stream today, pinned.
  * NativeConvTrainer: the eager step's weight gradients on ``wgrad_stream``, their operands alive at the join; the captured step
    single-stream.

What the trainer case does not see: aten ops issued from autograd's worker thread (allocations, ``.contiguous()`` copies, the loss
scale's multiply) are outside the TorchDispatchMode, which is per thread; the package's own launches and every wait are recorded on
that thread too (module patches), and the caching allocator's reuse of a freed block shows only as far as launches touch it."""
import dataclasses

import pytest
import torch

import stream_order as so
import swin_plan_cases as P
from stream_order import Region

pytestmark = pytest.mark.gpu
SMALLEST = min(P.CASES, key=lambda k: P.CASES[k]["N"] * P.CASES[k]["dims"][0] * P.CASES[k]["dims"][1] * P.CASES[k]["dims"][2])
MAIN_SCRATCH = {"raw1", "raw2", "res3", "splitk_ws", "_gemm_ws[0]"}
SIDE_SCRATCH = {"raw1b", "raw2b", "res3b", "splitk_ws_b", "_gemm_ws[1]"}
SIDE_BLOCKS = ("d1", "d2", "d3", "d4")                  # encoder1..4 of the denoiser: enc(0..3)
FLAT = {"raw1", "raw2", "res3", "raw1b", "raw2b", "res3b", "win", "att", "ln2", "merged", "qkv_buf", "hid_buf", "red_buf", "po_buf"}


def _names(plan):
    n = so.BufferNames().scan(plan)
    n.items = [it for it in n.items if not it[2].startswith("_tail_src")]         # views of raw2 / res3 / cat[0] under another name
    for r in plan.e_res + plan.d_res + plan.u_res:
        for k in range(3):
            n.add_tensor(f"{r.name}.st{k}", r.st[k])
    return n


def _report(what, rep):
    print(f"\n[{what}] {rep.summary()}")
    assert not rep.unordered, f"{what}: unordered conflicting launches:\n" + "\n".join(str(h) for h in rep.unordered[:12])


@pytest.fixture(scope="module")
def plans():
    from test_swin_launch_sequence_fp64 import _build
    cache = {}

    def get(case):
        if case not in cache:
            b = cache[case] = _build(case)
            b["tables"] = b["plan"]._step_tables(b["net"].sample_diffusion, "ddim", 0.0)
        return cache[case]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _step(b):
    from diff_unet_amos_amd import _native as nv
    coef, rows = b["tables"]
    b["plan"]._one_step(nv.MODE_DDIM, rows, coef, None, True)          # DDIM, in-kernel noise


def _start(b):
    plan = b["plan"]
    plan._reset(b["x"].float().contiguous())
    plan.new_seed(7)
    torch.cuda.synchronize()


def _record(b, steps=2, encoder=True, denoise=True):
    """One recording run: [run_encoder,] ``steps`` consecutive sampler steps [, one denoise]; marks between the phases."""
    plan = b["plan"]
    _start(b)
    with torch.no_grad(), so.Recorder(names=_names(plan)) as rec:
        if encoder:
            rec.mark("encoder")
            plan.run_encoder(b["image"])
        for k in range(steps):
            rec.mark(f"step{k}")
            _step(b)
        rec.mark("denoise")
        if denoise:
            plan.denoise(b["x"], b["t"])
        rec.mark("end")
    torch.cuda.synchronize()
    return rec.trace, _names(plan)


@pytest.fixture(scope="module")
def recorded(plans):
    cache = {}

    def get(case):
        if case not in cache:
            trace, names = _record(plans(case))
            cache[case] = (trace, names, so.analyse(trace, names))
        return cache[case]

    return get


def _kernels(records):
    return [r for r in so.launches(records) if r.kind == "launch"]


# ---- a. the Swin plans, eager ---------------------------------------------------------------------------------------------------------
def _tensor(plan, name):
    if "[" in name:
        attr, i = name[:-1].split("[")
        return getattr(plan, attr)[int(i)]
    return getattr(plan, name, None)


def _check_row(plan, names, L, row):
    """The recorded read and write sets of launch ``L`` against the operands tests/swin_plan_cases.py names for it."""
    reads, writes = {names.of(a.region) for a in L.reads}, {names.of(a.region) for a in L.writes}
    what = f"{row['name']} ({L.name})"
    src, off, c = row["src"]
    if not src.startswith("tmp."):
        assert src in reads, f"{what}: does not read {src}: {sorted(reads)}"
        t = _tensor(plan, src)
        if src not in FLAT:
            want = Region.channels(t, off, c)
            assert any(a.region == want for a in L.reads), f"{what}: no read of channels [{off}, {off + c}) of {src}"
        else:
            assert off == 0 and any(a.region.base == t.data_ptr() for a in L.reads), f"{what}: {src} is not read from its start"
    dst, doff = row["dst"]
    if not dst.startswith("tmp.") and dst != "logits":
        assert dst in writes, f"{what}: does not write {dst}: {sorted(writes)}"
        t = _tensor(plan, dst)
        if t is not None:
            at = t.data_ptr() + doff * t.element_size()
            assert any(a.region.base == at for a in L.writes), f"{what}: no write at channel offset {doff} of {dst}"
    for role, v in row["extra"].items():
        if role in ("norm", "res_norm"):
            assert v in reads, f"{what}: {role} {v} not read"
        elif role == "stats":
            assert v in writes, f"{what}: statistics {v} not accumulated"
        elif role == "t":
            assert "cur_add" in reads, f"{what}: the t_proj rows are not read"
        elif role == "x":
            assert v in writes, f"{what}: the fp32 stream {v} is not written"
        else:
            buf = v[0] if isinstance(v, tuple) else v
            if not buf.startswith("tmp."):
                assert buf in reads, f"{what}: {role} {buf} not read: {sorted(reads)}"
            if isinstance(v, tuple):
                t = _tensor(plan, buf)
                want = Region.channels(t, v[1], v[2] if len(v) > 2 else L_channels(L, t, v[1]))
                assert any(a.region == want for a in L.reads), f"{what}: {role} not read at channel offset {v[1]} of {buf}"


def L_channels(L, t, off):
    """channel count of the access of ``L`` that starts at channel ``off`` of ``t`` (rows of the table that give no count)"""
    at = t.data_ptr() + off * t.element_size()
    for a in L.reads:
        if a.region.base == at and a.region.rows > 1:
            return a.region.hi // t.element_size()
    return t.shape[-1] - off


def _check_step_shape(plan, names, case, seg, rep, trace, first="step_begin"):
    """One denoiser pass: ``first`` + the table's launches; streams, scratch sets, the join, the rows."""
    main, side = torch.cuda.current_stream().cuda_stream, plan.side_stream.cuda_stream
    ks = _kernels(seg)
    rows = P.sequence(case, "denoiser")
    assert ks[0].name == first and [k.name for k in ks[1:]] == [r["op"] for r in rows], \
        f"{case}: the recorded launches are not the table's: {[k.name for k in ks][:6]} ..."
    on_side = []
    for L, row in zip(ks[1:], rows):
        is_enc = row["name"].split(".")[0] in SIDE_BLOCKS
        assert L.stream == (side if is_enc else main), f"{case}: {row['name']} ({L.name}) on stream {L.stream:x}"
        _check_row(plan, names, L, row)
        on_side.append(L) if is_enc else None
    assert ks[0].stream == main and on_side
    for L in so.launches(seg, top=False):
        touched = {names.of(a.region) for a in L.reads + L.writes}
        bad = touched & (MAIN_SCRATCH if L.stream == side else SIDE_SCRATCH)
        assert L.stream in (main, side) and not bad, f"{case}: {L.name} on stream {L.stream:x} touches {bad}"
    # by the end of denoiser_body the main stream is ordered after every side launch: the tail is the next main-stream launch
    idx = {id(r): i for i, r in enumerate(trace)}
    tail = idx[id(ks[-1])]
    assert ks[-1].name == "final_conv_sampler" and ks[-1].stream == main
    late = [L.name for L in on_side if not rep.ordered(idx[id(L)], tail)]
    assert not late, f"{case}: side launches the tail is not ordered after: {late}"
    return len(on_side)


@pytest.mark.parametrize("case", list(P.CASES))
def test_swin_plan_eager_steps_are_ordered(case, plans, recorded):
    plan = plans(case)["plan"]
    trace, names, rep = recorded(case)
    _report(f"swin {case}: encoder + 2 steps + denoise", rep)
    main = torch.cuda.current_stream().cuda_stream
    assert plan.two_streams and set(rep.launches) == {main, plan.side_stream.cuda_stream}
    enc = _kernels(so.between(trace, "encoder", "step0"))
    rows = P.sequence(case, "encoder")
    assert [k.name for k in enc] == ["to_channels_last"] * 2 + [r["op"] for r in rows] and all(k.stream == main for k in enc)
    assert not so.syncs(so.between(trace, "encoder", "step0"))
    for L, row in zip(enc[2:], rows):
        _check_row(plan, names, L, row)
    n0 = _check_step_shape(plan, names, case, so.between(trace, "step0", "step1"), rep, trace)
    n1 = _check_step_shape(plan, names, case, so.between(trace, "step1", "denoise"), rep, trace)
    den = so.between(trace, "denoise", "end")
    k = next(i for i, r in enumerate(den) if isinstance(r, so.Launch) and r.name == "step_begin")
    assert [r.name for r in _kernels(den[:k])] == ["to_channels_last"]
    n2 = _check_step_shape(plan, names, case, den[k:], rep, trace)
    assert n0 == n1 == n2
    # per pass: one fork (wait_stream), one record per encoder block, one wait per block
    for a, b in (("step0", "step1"), ("step1", "denoise"), ("denoise", "end")):
        kinds = [s.kind for s in so.syncs(so.between(trace, a, b))]
        assert sorted(kinds) == ["record"] * 4 + ["wait_event"] * 4 + ["wait_stream"], kinds


# ---- b. the order knobs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", ["conv3_first", "side_plan_a", "side_plan_b", "one_stream"])
def test_swin_order_knobs_stay_ordered(knob, plans):
    b = plans(SMALLEST)
    plan = b["plan"]
    saved = (plan.conv3_first, plan.side_plan, plan.two_streams)
    try:
        if knob == "conv3_first":
            plan.conv3_first = True
        elif knob == "side_plan_a":
            plan.side_plan = {1: (3,), 2: (2, 1, 0)}
        elif knob == "side_plan_b":
            plan.side_plan = {0: (0,), 1: (1,), 2: (3, 2)}
        else:
            plan.two_streams = False
        trace, names = _record(b, encoder=False, denoise=False)
    finally:
        plan.conv3_first, plan.side_plan, plan.two_streams = saved
    rep = so.analyse(trace, names)
    _report(f"swin {SMALLEST} {knob}: 2 steps", rep)
    main, side = torch.cuda.current_stream().cuda_stream, plan.side_stream.cuda_stream
    rows = P.sequence(SMALLEST, "denoiser")
    for seg in (so.between(trace, "step0", "step1"), so.between(trace, "step1", "denoise")):
        ks = _kernels(seg)
        assert len(ks) == 1 + len(rows) and sorted(k.name for k in ks[1:]) == sorted(r["op"] for r in rows)
        if knob == "one_stream":
            assert not so.syncs(seg) and all(L.stream == main for L in so.launches(seg, top=False))
        else:
            # side_plan_a lists block 3 (encoder4, which reads hs[2]) at stage 1: the plan starts it once hs[2] is enqueued, with
            # the blocks of stage 2 -- one fork.  (Launched at stage 1 it read hs[2] unordered against this step's stage_out.)
            forks = {"conv3_first": 1, "side_plan_a": 1, "side_plan_b": 3}[knob]
            assert sorted(s.kind for s in so.syncs(seg)) == ["record"] * 4 + ["wait_event"] * 4 + ["wait_stream"] * forks
            assert sum(L.stream == side for L in ks) == sum(r["name"].split(".")[0] in SIDE_BLOCKS for r in rows)
    if knob == "one_stream":
        assert set(rep.launches) == {main} and rep.examined == 0
    if knob == "conv3_first":                # conv3 (the block's only launch on its input alone) leads each side block that has one
        ks = [k.name for k in _kernels(so.between(trace, "step0", "step1")) if k.stream == side]
        assert ks[-3:] == ["conv3d_k3", "conv3d_k3", "residual_norm_act"] and ks[-4] in ("instnorm_stats", "token_linear"), ks[-6:]


# ---- c. the captured step ---------------------------------------------------------------------------------------------------------------
def test_swin_capture_pass_issues_the_eager_trace(plans, recorded):
    b = plans(SMALLEST)
    plan = b["plan"]
    eager, _, _ = recorded(SMALLEST)
    _start(b)
    n = [0]
    with torch.no_grad(), so.Recorder(names=_names(plan)) as rec:

        def step_fn():
            rec.mark(f"pass{n[0]}")
            _step(b)
            rec.mark(f"pass{n[0]}end")
            n[0] += 1

        g = plan.capture_step(step_fn)          # warm-up pass, synchronize, capture pass; never replayed here
    torch.cuda.synchronize()
    assert n[0] == 2
    del g
    want = so.shape_of(so.between(eager, "step1", "denoise"))
    warm, cap = so.shape_of(so.between(rec.trace, "pass0", "pass0end")), so.shape_of(so.between(rec.trace, "pass1", "pass1end"))
    assert len(want) > 100 and any(r[0] == "wait_stream" for r in want)
    assert warm == want, "the warm-up pass differs from the eager step"
    assert cap == want, "the capture pass differs from the eager step: " + str(next((a, b) for a, b in zip(cap, want) if a != b))
    capture_stream = next(r for r in so.between(rec.trace, "pass1", "pass1end") if isinstance(r, so.Launch)).stream
    assert capture_stream != torch.cuda.current_stream().cuda_stream           # the pass did run under the capture
    _report(f"swin {SMALLEST}: warm-up + capture pass", so.analyse(rec.trace, _names(plan)))


# ---- d. planted defects, on the recorded trace only ------------------------------------------------------------------------------------
def _steps_only(trace):
    i = next(k for k, r in enumerate(trace) if isinstance(r, so.Note) and r.label == "step0")
    j = next(k for k, r in enumerate(trace) if isinstance(r, so.Note) and r.label == "denoise")
    return trace[i:j]


def test_planted_defects_in_the_recorded_swin_trace_are_reported(plans, recorded):
    plan = plans(SMALLEST)["plan"]
    full, names, rep = recorded(SMALLEST)
    trace = _steps_only(full)
    main, side = torch.cuda.current_stream().cuda_stream, plan.side_stream.cuda_stream
    assert not rep.unordered and not so.analyse(trace, names).unordered
    found = lambda t: [(h.kind, h.first.name, h.first.stream, h.second.stream, h.buffer) for h in so.analyse(t, names).unordered]  # noqa: E731

    # 1. the decoder no longer waits for enc_done[2]
    ev = next(i for i, r in enumerate(trace) if isinstance(r, so.Sync) and r.kind == "wait_event" and r.event == id(plan.enc_done[2]))
    got = found(trace[:ev] + trace[ev + 1:])
    print("\nwithout wait_event(enc_done[2]):", got[:4])
    assert ("RAW", "residual_norm_act", side, main, "cat[2]") in got

    # 2. the side stream no longer waits for the main stream in ready(2)
    ws = next(i for i, r in enumerate(trace) if isinstance(r, so.Sync) and r.kind == "wait_stream" and r.stream == side)
    got = found(trace[:ws] + trace[ws + 1:])
    print("without side.wait_stream(main):", sorted({g[4] for g in got}))
    raw = {g[4] for g in got if g[0] == "RAW" and g[2] == main and g[3] == side}
    assert raw & {"hs[0]", "hs[1]", "hs[2]", "xin"} and {"hs[1]"} <= raw

    # 3. the side block on the main chain's raw1
    shift = plan.raw1.data_ptr() - plan.raw1b.data_ptr()
    lo, hi = Region.of_tensor(plan.raw1b).hull()

    def moved(accs):
        return [so.Access(dataclasses.replace(a.region, base=a.region.base + shift), a.role) if lo <= a.region.base < hi else a
                for a in accs]

    edited = [so.Launch(r.name, r.stream, moved(r.reads), moved(r.writes), r.label, r.depth, r.kind)
              if isinstance(r, so.Launch) and r.stream == side else r for r in trace]
    got = found(edited)
    print("side block on raw1:", got[:4])
    assert any(g[0] in ("WAW", "WAR") and g[4] == "raw1" and {g[2], g[3]} == {main, side} for g in got)


# ---- e. the DiffUNet plan: single-stream today --------------------------------------------------------------------------------------------
def test_diffunet_plan_steps_on_one_stream():
    from diff_unet_amos_amd import _native as nv
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from test_diffunet_gpu import TINY
    torch.manual_seed(0)
    net = DiffUNet(**TINY).cuda().eval()
    dev = torch.device("cuda", 0)
    plan = net._rt.plan(1, (32, 32, 32), dev)
    g = torch.Generator().manual_seed(1)
    image, x = torch.rand(1, 1, 32, 32, 32, generator=g).cuda(), torch.randn(1, TINY["out_channels"], 32, 32, 32, generator=g).cuda()
    with torch.no_grad():
        plan.run_encoder(image)
        coef, rows = plan._step_tables(net.sample_diffusion, "ddim", 0.0)
        plan._reset(x)
        plan.new_seed(3)
        torch.cuda.synchronize()
        names = so.BufferNames().scan(plan)
        with so.Recorder(names=names) as rec:
            for _ in range(2):
                plan._one_step(nv.MODE_DDIM, rows, coef, None, True)
    torch.cuda.synchronize()
    rep = so.analyse(rec.trace, names)
    _report("diffunet tiny 32^3: 2 steps", rep)
    ls = so.launches(rec.trace, top=False)
    main = torch.cuda.current_stream().cuda_stream
    assert sum(L.name == "denoiser_step" for L in ls) == 2 and all(L.stream == main for L in ls)
    assert all(L.reads and L.writes for L in ls if L.name == "denoiser_step")
    assert not so.syncs(rec.trace) and rep.examined == 0 and set(rep.launches) == {main}


# ---- f. the trainer ---------------------------------------------------------------------------------------------------------------------
def _trainer(graph):
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    from test_diffunet_gpu import TINY
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    net = DiffUNet(**TINY).to(dev)
    tr = NativeConvTrainer(net, lr=1e-3, dtype=torch.float16, graph=graph)
    tr.n_conv = sum(isinstance(m, torch.nn.Conv3d) and tuple(m.kernel_size) == (3, 3, 3) for m in net.modules())
    g = torch.Generator().manual_seed(2)
    images = torch.rand(2, 1, 32, 32, 32, generator=g).to(dev)
    labels = (torch.rand(2, TINY["out_channels"], 32, 32, 32, generator=g) > 0.5).float().to(dev)
    noise = [torch.randn(2, TINY["out_channels"], 32, 32, 32, generator=g).to(dev) for _ in range(2)]
    t = [torch.tensor([500, 37]).to(dev), torch.tensor([3, 999]).to(dev)]
    return tr, images, labels, noise, t


def test_trainer_eager_weight_gradients_on_the_side_stream_are_ordered():
    """Two consecutive eager steps.  Not seen: aten ops issued from autograd's worker thread (the TorchDispatchMode is per thread);
    every launch of the package and every wait on that thread is."""
    from diff_unet_amos_amd import ops
    tr, images, labels, noise, t = _trainer(False)
    assert tr.wgrad_stream is not None
    main, side = torch.cuda.current_stream().cuda_stream, tr.wgrad_stream.cuda_stream
    torch.cuda.synchronize()
    names = so.BufferNames()
    names.add_tensor("arena", tr.arena.buf)
    owners = lambda: [tr.arena.buf] + [p.grad for p in tr.params]  # noqa: E731
    with so.Recorder(names=names, liveness=("conv3d_k3_wgrad",), owners=owners) as rec:
        for k in range(2):
            rec.mark(f"step{k}")
            tr.step(images, labels, noise=noise[k], t=t[k])
        rec.mark("end")
    torch.cuda.synchronize()
    trace = rec.trace
    for (dev, h), buf in list(ops._WGRAD_WS.items()) + list(ops._SPLITK_WS.items()):
        names.add_tensor(f"ws@{h:x}", buf)
    rep = so.analyse(trace, names)
    _report("trainer tiny 32^3 fp16 eager: 2 steps", rep)
    idx = {id(r): i for i, r in enumerate(trace)}
    ls = so.launches(trace, top=False)
    wg = [L for L in ls if L.name == "conv3d_k3_wgrad"]
    assert tr.n_conv > 0 and len(wg) == 2 * tr.n_conv and all(L.stream == side for L in wg), (len(wg), {L.stream for L in wg})
    assert all(L.stream == main for L in ls if L.name != "conv3d_k3_wgrad") and set(rep.launches) == {main, side}
    # every weight gradient is ordered after the launches that produced its x and its dy
    for L in wg:
        j = idx[id(L)]
        for role in ("x", "dy"):
            mine = [a for a in L.reads if a.role == role]
            prod = [idx[id(M)] for M in ls if M.stream != side and idx[id(M)] < j and so._first_conflict(M.writes, mine)]
            assert prod and all(rep.ordered(i, j) for i in prod), f"{role} of the weight gradient at {j}: producers {prod}"
    # the join precedes the first read of dw (grads_nonfinite / adamw_step) and the next step's arena reset
    resets = [idx[id(L)] for L in ls if L.name == "aten::zero_" and any(a.region == Region.of_tensor(tr.arena.buf) for a in L.writes)]
    assert len(resets) == 2
    for k, (a, b) in enumerate((("step0", "step1"), ("step1", "end"))):
        seg = so.between(trace, a, b)
        mine = [L for L in seg if isinstance(L, so.Launch) and L.name == "conv3d_k3_wgrad"]
        joins = [r for r in seg if isinstance(r, so.Sync) and r.kind == "wait_stream" and r.stream == main and r.other == side]
        assert len(mine) == tr.n_conv and len(joins) == 1
        readers = [L for L in seg if isinstance(L, so.Launch) and L.name in ("grads_nonfinite", "adamw_step")]
        assert readers and idx[id(joins[0])] < idx[id(readers[0])]
        for L in mine:
            dw = [a for a in L.writes if a.role == "dw"]
            users = [M for M in readers if so._first_conflict(M.reads, dw)]
            assert users and all(rep.ordered(idx[id(L)], idx[id(M)]) for M in users)
            assert rep.ordered(resets[k], idx[id(L)])                       # the zero fill of its accumulator
            if k == 0:
                assert rep.ordered(idx[id(L)], resets[1])                   # the next step's reuse of the arena
    # the two streams' workspaces are distinct buffers
    ws = lambda s: [a.region for L in ls if L.stream == s for a in L.writes if a.role in ("_wgrad_ws", "splitk_ws", "workspace")]  # noqa: E731
    assert ws(main) and not any(a.conflicts(b) for a in set(ws(side)) for b in set(ws(main)))
    for cache in (ops._WGRAD_WS, ops._SPLITK_WS):
        bufs = [Region.of_tensor(buf) for (_, h), buf in cache.items() if h in (main, side)]
        assert not any(a.conflicts(b) for i, a in enumerate(bufs) for b in bufs[i + 1:])
    # liveness: the tensor objects x and dy of every side launch are alive at the join (what _WGRAD["keep"] is for).  dw is handed to
    # autograd, which keeps the memory under a tensor object of its own (param.grad) and lets go of the one the launch was given:
    # for dw the object may be gone, and then its bytes must lie in the trainer's arena or in a parameter's gradient at the join
    notes = [r for r in trace if isinstance(r, so.Note) and r.kind == "liveness"]
    assert len(notes) == 3 * len(wg) and {n.data["role"] for n in notes} == {"x", "dy", "dw"}
    dead = [(n.data["role"], idx[id(n.data["launch"])]) for n in notes
            if not (n.data["alive"] or (n.data["role"] == "dw" and n.data["owned"]))]
    assert not dead, f"operands of side-stream weight gradients freed before the join: {dead[:8]}"
    print(f"liveness at the joins: {sum(n.data['alive'] for n in notes)} of {len(notes)} operand objects alive, "
          f"{sum(not n.data['alive'] and n.data['owned'] for n in notes)} dw accumulators owned by the arena / param.grad")


def test_trainer_captured_step_is_single_stream():
    tr, images, labels, _, _ = _trainer(True)
    assert tr.wgrad_stream is None and tr.capture_stream is not None
    torch.cuda.synchronize()
    body, n = tr._graph_body, [0]
    with so.Recorder() as rec:

        def marked():
            rec.mark(f"body{n[0]}")
            n[0] += 1
            try:
                return body()
            finally:
                rec.mark(f"body{n[0] - 1}end")

        tr._graph_body = marked
        try:
            tr._build_graph(images, labels)         # three warm-up bodies on the capture stream, then the capture; no replay
        finally:
            del tr._graph_body
    torch.cuda.synchronize()
    assert n[0] == 4
    cap = so.between(rec.trace, "body3", "body3end")
    ls = so.launches(cap, top=False)
    assert len(ls) > 100 and {L.stream for L in ls} == {tr.capture_stream.cuda_stream}
    assert sum(L.name == "conv3d_k3_wgrad" for L in ls) == tr.n_conv and not so.syncs(cap)
    rep = so.analyse(cap)
    _report("trainer tiny 32^3 fp16: the capture pass", rep)
    assert rep.examined == 0
