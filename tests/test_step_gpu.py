"""The sampler step's own kernels and its one-call entry point on the GPU (csrc/temb.hip, csrc/denoiser_step.hip), against
tests/step_ref.py.

1. step_begin_kernel, exact: every buffer it reads or writes is a slice in the middle of a larger allocation whose guard entries
   hold sentinels (for row_of_step: valid rows that no step uses), so a read that missed its clamp shows as a sentinel in cur_add /
   cur_coef and a write past an end as a damaged guard.  Planted out-of-range indices stay within one guard of the range (-1,
   table_rows, nsteps).  The kernel clamps every index before the read that depends on it; these are contract tests.
2. temb_table_kernel: (a) bit-equal to the block-major ``add`` of dua_temb_train_fwd (which is held stage by stage to float64,
   tests/glue_fp64ref.py) and (b) within step_ref.temb_table_ref's propagated bound of the chained float64 evaluation.
3. Plan.native_step (dua_denoiser_step executing the recorded op list) leaves the same bits as step_begin + denoiser_body() +
   tail() launched one by one, in every buffer of the plan; and the recorded convolution descriptors are the ones
   tests/conv_form_cases.plan_launches writes by hand (tests/test_conv3_form.py pins their launch forms).
4. The argument checks of the three entry points on real tensors: the valid argument set launches and does its work, the same set
   with one bad argument returns ERR_ARG and writes nothing (the lists of tests/step_ref.py, which tests/test_step_ref.py applies
   to made-up addresses without a device).

Figures are printed before they are asserted (run with -s); the module prints one line per temb layout at its end."""
import ctypes as C

import pytest
import torch

import conv_form_cases as K
import glue_fp64ref as GR
import step_ref as SR
from test_glue_fp64 import LAYOUTS
from test_launch_sequence_fp64 import EXPECTED, TIMESTEPS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32
NAN = float("nan")
SENT, T_SENT, C_SENT, I_SENT = 777.25, -911.5, -655.75, 0x5A5A5A5       # output guards; table guards; coefficient guards; int guards
GUARD = 64
TABLE_ROWS = 7                      # rows 0..4 are used by steps, 5 and 6 only by the guard entries of row_of_step
TEMB_LINES = {}


def _ops():
    from diff_unet_amos_amd import ops
    return ops


def _nv():
    from diff_unet_amos_amd import _native
    return _native


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(-1).view(torch.uint8),
                                                                          b.contiguous().view(-1).view(torch.uint8)))


def _guarded(n, fill=NAN, lead=0, dtype=F32, sent=SENT):
    """(whole buffer, the n-element payload ``lead`` words past the first guard): guards hold ``sent``, the payload ``fill``."""
    buf = torch.full((GUARD + lead + n + GUARD,), sent, dtype=dtype, device=DEV)
    view = buf[GUARD + lead:GUARD + lead + n]
    view.fill_(fill)
    return buf, view


def _guards_intact(buf, view, sent=SENT):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == sent).all()) and bool((buf[lo + view.numel():] == sent).all())


# ---- 1. step_begin ----------------------------------------------------------------------------------------------------------------------
class _Begin:
    """The operands of step_begin launches: inputs between one-entry guards (a whole row of sentinels either side of the table and
    of the coefficient table, a valid unused row either side of row_of_step), outputs NaN-filled between guard words, the three
    device words apart from each other inside one int32 buffer of sentinels."""

    def __init__(self, N, P, nsteps=0, row_of_step=None, counter=0):
        self.N, self.P, self.nsteps = N, P, nsteps
        rows = TABLE_ROWS
        self.tbuf = torch.full(((rows + 2) * P,), T_SENT, dtype=F32, device=DEV)
        self.table = self.tbuf[P:(rows + 1) * P].view(rows, P)
        self.table.copy_((torch.arange(rows, dtype=F32)[:, None] * 4096 + torch.arange(P, dtype=F32)[None, :] + 0.5).to(DEV))
        nc = max(nsteps, 1)
        self.cbuf = torch.full(((nc + 2) * 8,), C_SENT, dtype=F32, device=DEV)
        self.coef = self.cbuf[8:(nc + 1) * 8].view(nc, 8)
        self.coef.copy_(-(torch.arange(nc * 8, dtype=F32).view(nc, 8) + 1).to(DEV))
        self.ros = None
        if nsteps:
            self.rbuf = torch.tensor([5, *row_of_step, 6], dtype=I32, device=DEV)
            self.ros = self.rbuf[1:1 + nsteps]
        self.abuf, self.cur_add = _guarded(N * P)
        self.kbuf, self.cur_coef = _guarded(N * 8)
        self.ibuf = torch.full((48,), I_SENT, dtype=I32, device=DEV)
        self.counter, self.step_word, self.err_word = self.ibuf[8:9], self.ibuf[24:25], self.ibuf[40:41]
        self.counter.fill_(counter)
        self.step_word.fill_(-77)
        self.err_word.zero_()
        self.inputs = [(b, b.clone()) for b in (self.tbuf, self.cbuf) + ((self.rbuf,) if nsteps else ())]
        self.want_add = torch.full((N, P), NAN)
        self.want_coef = torch.full((N, 8), NAN)
        self.want = dict(counter=counter, step_word=-77, err=0)

    def expect(self, rows_per_sample=None, coef=True, step_word=True, err_word=True):
        """Advance the expectation by one launch (step_ref.step_begin_ref on host copies)."""
        r = SR.step_begin_ref(self.N, self.table.cpu(), rows_per_sample=rows_per_sample,
                              row_of_step=None if rows_per_sample is not None else self.ros.cpu().tolist(),
                              counter=self.want["counter"], coef_table=self.coef.cpu() if coef else None)
        self.want_add = r["cur_add"]
        if coef:
            self.want_coef = r["cur_coef"]
        if rows_per_sample is None:
            self.want["counter"] = r["counter"]
            if step_word:
                self.want["step_word"] = r["step_word"]
        if r["err"] and err_word:
            self.want["err"] = 1
        return r

    def check(self, what):
        got = dict(counter=int(self.counter), step_word=int(self.step_word), err=int(self.err_word))
        assert got == self.want, (what, got, self.want)
        assert torch.equal(self.cur_add.view(self.N, self.P).cpu(), self.want_add), f"{what}: cur_add"
        if bool(torch.isnan(self.want_coef).all()):
            assert bool(torch.isnan(self.cur_coef).all()), f"{what}: cur_coef was written"
        else:
            assert torch.equal(self.cur_coef.view(self.N, 8).cpu(), self.want_coef), f"{what}: cur_coef"
        assert _guards_intact(self.abuf, self.cur_add) and _guards_intact(self.kbuf, self.cur_coef), f"{what}: output guards"
        words = torch.ones(48, dtype=torch.bool)
        words[[8, 24, 40]] = False
        assert bool((self.ibuf.cpu()[words] == I_SENT).all()), f"{what}: a word next to counter / step_word / err_word"
        for buf, keep in self.inputs:
            assert torch.equal(buf, keep), f"{what}: an input was written"

    def launch(self, rows_per_sample=None, coef=True, step_word=True, err_word=True, clear=None, c_entry=False):
        ops, nv = _ops(), _nv()
        rows = None if rows_per_sample is None else torch.tensor(rows_per_sample, dtype=I32, device=DEV)
        kw = dict(rows_per_sample=rows, row_of_step=self.ros, counter=self.counter, coef_table=self.coef if coef else None,
                  cur_coef=self.cur_coef, step_word=self.step_word if step_word else None,
                  err_word=self.err_word if err_word else None)
        if not c_entry:
            ops.step_begin(self.N, self.table, self.cur_add, clear=clear, **kw)
            return
        assert clear is None
        rc = nv.lib().dua_step_begin_clear(self.N, self.P, nv.ptr(self.table), TABLE_ROWS, nv.ptr(rows), nv.ptr(self.ros), self.nsteps,
                                           nv.ptr(kw["coef_table"]), nv.ptr(self.counter), nv.ptr(self.cur_add), nv.ptr(self.cur_coef),
                                           nv.ptr(kw["step_word"]), nv.ptr(kw["err_word"]), None, 0, nv.stream_ptr())
        assert rc == 0


ROW_VECTORS = {1: [[0], [TABLE_ROWS - 1], [2], [-1], [TABLE_ROWS]],
               3: [[TABLE_ROWS - 1, 0, TABLE_ROWS - 1], [2, 2, 3], [-1, 3, 0], [1, TABLE_ROWS, 1], [TABLE_ROWS, 0, -1]]}


@pytest.mark.parametrize("P", [8, 255, 256, 257, 1544])
@pytest.mark.parametrize("N", [1, 3])
def test_step_begin_rows_per_sample(N, P):
    """Rows first, last, repeated, one below and one above the table; counter and step_word are handed over and stay as they
    were; row 0 of the coefficient table lands in every sample's cur_coef (k = 0), and without a table cur_coef is not written."""
    for rows in ROW_VECTORS[N]:
        for coef in (True, False):
            s = _Begin(N, P, counter=41)
            r = s.expect(rows_per_sample=rows, coef=coef)
            assert r["err"] == any(not 0 <= x < TABLE_ROWS for x in rows)
            s.launch(rows_per_sample=rows, coef=coef)
            s.check(f"N {N} P {P} rows {rows} coef {coef}")
            assert s.want["counter"] == 41 and s.want["step_word"] == -77
            if coef:
                assert torch.equal(s.cur_coef.view(N, 8).cpu(), s.coef[0].cpu().expand(N, 8))


PLANTS = {1: [None, {0: -1}, {0: TABLE_ROWS}], 5: [None, {1: -1, 3: TABLE_ROWS}]}
COUNTER_CASES = [(nsteps, N, plant, start) for nsteps in (1, 5) for N in (1, 2) for plant in PLANTS[nsteps] for start in (0, -1)
                 if plant is None or start == 0]


def _row_of_step(nsteps, plant):
    ros = [4, 2, 2, 0, 3][:nsteps]
    for i, v in (plant or {}).items():
        ros[i] = v
    return ros


def _run_counter_launches(s, launches, what, **kw):
    """Launch by launch: the expectation advanced, the launch, everything compared; yields (launch, what the reference said)."""
    for j in range(launches):
        r = s.expect(**{k: v for k, v in kw.items() if k != "c_entry"})
        s.launch(**kw)
        s.check(f"{what} launch {j}")
        yield j, r


@pytest.mark.parametrize("nsteps,N,plant,start", COUNTER_CASES)
def test_step_begin_counter_mode(nsteps, N, plant, start):
    """nsteps + 2 launches in a row: step_word = min(j, nsteps - 1), counter one more, the step's row and coefficients in every
    sample, the error word 0 through launch nsteps - 1 and 1 from launch nsteps on (sooner where the counter starts at -1 or a
    planted row is met: it is never cleared by the kernel)."""
    P = 257
    s = _Begin(N, P, nsteps, _row_of_step(nsteps, plant), counter=start)
    for j, r in _run_counter_launches(s, nsteps + 2, f"nsteps {nsteps} N {N} plant {plant} start {start}"):
        k = min(j, nsteps - 1)
        assert (s.want["step_word"], s.want["counter"]) == (k, k + 1)
        if plant is None and start == 0:
            assert s.want["err"] == (1 if j >= nsteps else 0)
        if start == -1:
            assert s.want["err"] == 1 and (j > 0 or r["err"])
        if plant is not None and j <= min(plant):
            assert s.want["err"] == (1 if j == min(plant) else 0)
    assert s.want["err"] == 1


@pytest.mark.parametrize("null", ["step_word", "err_word", "coef_table"])
@pytest.mark.parametrize("nsteps", [1, 5])
def test_step_begin_counter_mode_null_outputs(nsteps, null):
    """Through the C entry point with one optional pointer NULL: what it names is not written, the rest goes on as before."""
    s = _Begin(2, 257, nsteps, _row_of_step(nsteps, {nsteps - 1: TABLE_ROWS}))
    kw = dict(step_word=null != "step_word", err_word=null != "err_word", coef=null != "coef_table", c_entry=True)
    for _ in _run_counter_launches(s, nsteps + 2, f"nsteps {nsteps} without {null}", **kw):
        pass
    assert s.want["counter"] == nsteps and s.want["err"] == (0 if null == "err_word" else 1)
    assert s.want["step_word"] == (-77 if null == "step_word" else nsteps - 1)


def test_step_begin_counter_mode_in_a_captured_graph():
    """One launch captured after a warm-up launch, replayed nsteps + 1 times: the sequence of the eager launches, the counter
    going on from where the warm-up left it.  (A one-node graph: nothing runs in parallel.)"""
    nsteps, N = 5, 2
    s = _Begin(N, 257, nsteps, _row_of_step(nsteps, None))
    s.expect()
    s.launch()
    torch.cuda.synchronize()
    s.check("warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.launch()
    s.check("capture launches nothing")
    for j in range(1, nsteps + 2):
        s.expect()
        g.replay()
        torch.cuda.synchronize()
        s.check(f"replay {j}")
        assert s.want["step_word"] == min(j, nsteps - 1) and s.want["err"] == (1 if j >= nsteps else 0)
    assert s.want["counter"] == nsteps


@pytest.mark.parametrize("pieces", [0, 1, 1024, 1024 * 1024 + 3])
def test_step_begin_clears_the_arena(pieces):
    """``pieces`` sixteen-byte pieces of 3.5 between guard words, 16 bytes into a guarded buffer: all zero bits afterwards, the
    guards as they were, the row copy done.  1024 * 1024 + 3 pieces are past the cap of 1024 clearing blocks: the grid-stride loop
    runs a fifth time for three threads.  0 pieces: one block, nothing cleared."""
    s = _Begin(3, 257)
    buf, arena = _guarded(4 * pieces + 8, 3.5, lead=4)
    assert arena.data_ptr() % 16 == 0
    clear, rest = arena[:4 * pieces], arena[4 * pieces:]
    rows = [TABLE_ROWS - 1, 0, 3]
    s.expect(rows_per_sample=rows)
    s.launch(rows_per_sample=rows, clear=clear)
    s.check(f"clear {pieces} pieces")
    assert bool((clear.view(I32) == 0).all()), "a word of the arena was not cleared"
    assert bool((rest == 3.5).all()) and _guards_intact(buf, arena), "the clear went past the arena"


# ---- 2. temb_table ----------------------------------------------------------------------------------------------------------------------------
EDGE_TIMESTEPS = [0, 1, 2, 499, 998, 999]
SWIN = [("swin48", 64, SR.swin_blocks(48)), ("swin12", 64, SR.swin_blocks(12))]
TEMB_LAYOUTS = [(n, h, [(c, False) for c in couts]) for n, h, couts in LAYOUTS] + SWIN


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if TEMB_LINES:
        print("\ntemb_table per layout: largest |err| / bound against the chained fp64 reference; bit-equal to temb_train_fwd")
        for name, (ratio, same) in sorted(TEMB_LINES.items()):
            print(f"  {name:<14} {ratio:.3e}  {'bit-equal' if same else 'DIFFERS'}")


def _temb_case(layout, hid, timesteps, seed=3):
    name, half, blocks = layout
    w0, b0, w1, b1, ws, bs = SR.make_layout_params(hid, half, blocks, seed, DEV)
    return dict(half=half, hid=hid, t=torch.tensor(timesteps, dtype=torch.int64, device=DEV), freqs=GR.temb_freqs(half).to(DEV),
                w0=w0, b0=b0, w1=w1, b1=b1, ws=ws, bs=bs, wcat=torch.cat(ws, 0).contiguous(), bcat=torch.cat(bs, 0).contiguous(),
                couts=[w.shape[0] for w in ws], pads=SR.pad_mask(blocks))


def _table(c, t=None):
    """ops.temb_table into a NaN-filled [T, P] view between guard words."""
    t = (c["t"] if t is None else t).to(I32).contiguous()
    T, P = t.numel(), c["wcat"].shape[0]
    buf, flat = _guarded(T * P)
    out = _ops().temb_table(t, c["freqs"], c["w0"], c["b0"], c["w1"], c["b1"], c["wcat"], c["bcat"], out=flat.view(T, P))
    assert out.data_ptr() == flat.data_ptr() and _guards_intact(buf, flat), "temb_table wrote outside its table"
    assert bool(torch.isfinite(out).all()), "a table word is not finite (or was not written)"
    return out


def _train_forward(c, lo, hi):
    """dua_temb_train_fwd over blocks [lo, hi) (at most 16 per call): (rows [N, sum cout], saved [N, 2 half + 4 hid])."""
    nv, ops = _nv(), _ops()
    ws, bs, couts = c["ws"][lo:hi], c["bs"][lo:hi], c["couts"][lo:hi]
    N, half, hid = c["t"].numel(), c["half"], c["hid"]
    width = 2 * half + 4 * hid
    abuf, add = _guarded(N * sum(couts))
    sbuf, saved = _guarded(N * width)
    rc = nv.lib().dua_temb_train_fwd(N, nv.ptr(c["t"]), nv.ptr(c["freqs"]), half, hid, nv.ptr(c["w0"]), nv.ptr(c["b0"]), nv.ptr(c["w1"]),
                                     nv.ptr(c["b1"]), C.byref(ops._temb_blocks(ws, bs=bs)), nv.ptr(add), nv.ptr(saved), nv.stream_ptr())
    assert rc == 0 and _guards_intact(abuf, add) and _guards_intact(sbuf, saved)
    saved = saved.view(N, width)
    ref = GR.temb_fwd_ref(c["t"], c["freqs"], c["w0"], c["b0"], c["w1"], c["b1"], ws, bs, saved)
    res = GR.temb_fwd_checks(add, saved, ref, half, hid)
    return SR.rows_of_block_major(add, N, couts), saved, res


def _against_fp64(c, table, t=None):
    cpu = lambda x: x.cpu()          # noqa: E731
    t = c["t"] if t is None else t
    ref, bound = SR.temb_table_ref(cpu(t), cpu(c["freqs"]), cpu(c["w0"]), cpu(c["b0"]), cpu(c["w1"]), cpu(c["b1"]), cpu(c["wcat"]),
                                   cpu(c["bcat"]))
    return GR.check(table.cpu(), ref, bound)


@pytest.mark.parametrize("hid", [256, 512])
@pytest.mark.parametrize("layout", TEMB_LAYOUTS, ids=[l[0] for l in TEMB_LAYOUTS])
def test_temb_table_equals_the_training_forward_and_fp64(layout, hid):
    """(a) the table's rows are the training forward's ``add`` bit for bit, with the training forward's stages and ``add`` inside
    glue_fp64ref's bounds on what each stage read; (b) the table is inside step_ref.temb_table_ref's propagated bound of the chained
    float64 evaluation; the padded columns of the Swin layout are exactly 0.0; t = 0 (e = [0 | 1]), 1, 2, 499, 998, 999."""
    name = f"{layout[0]}/{hid}"
    c = _temb_case(layout, hid, EDGE_TIMESTEPS)
    table = _table(c)
    rows, stage_res, saved = [], {}, None
    for lo in range(0, len(c["ws"]), 16):
        r, saved, res = _train_forward(c, lo, min(lo + 16, len(c["ws"])))
        rows.append(r)
        for k, v in res.items():
            if k not in stage_res or v.ratio > stage_res[k].ratio:
                stage_res[k] = v
    twin = torch.cat(rows, 1)
    same = _same_bits(table, twin)
    fp64 = _against_fp64(c, table)
    TEMB_LINES[name] = (fp64.ratio, same)
    worst = max(stage_res.items(), key=lambda kv: kv[1].ratio)
    print(f"temb_table {name}: against fp64 {fp64}; bit-equal to temb_train_fwd: {same}; training forward worst {worst[0]} {worst[1]}")
    half = c["half"]
    assert torch.equal(saved[0, :2 * half].cpu(), torch.cat([torch.zeros(half), torch.ones(half)])), "t = 0: e = [0 | 1]"
    for k, v in stage_res.items():
        assert v.ratio <= 1.0, (name, "temb_train_fwd", k, v)
    if not same:
        d = (table != twin).nonzero()
        assert same, f"{name}: {len(d)} table words differ from temb_train_fwd, first at {d[0].tolist()}: " \
                     f"{float(table[tuple(d[0])])!r} against {float(twin[tuple(d[0])])!r}"
    assert fp64.ratio <= 1.0, (name, fp64)
    if bool(c["pads"].any()):
        assert bool((table[:, c["pads"].to(DEV)].view(I32) == 0).all()), f"{name}: a padded column is not +0.0"


def test_temb_table_rows_do_not_depend_on_their_place():
    """An unordered list with a repeat: the two rows of the repeated timestep are bit-equal, and every row equals the one the
    ordered launch of the same layout computes for that timestep."""
    layout = TEMB_LAYOUTS[0]
    ts = [999, 2, 499, 2, 0]
    c = _temb_case(layout, 512, ts)
    table = _table(c)
    assert _same_bits(table[1], table[3])
    ordered = _table(c, torch.tensor(EDGE_TIMESTEPS, device=DEV))
    for i, t in enumerate(ts):
        assert _same_bits(table[i], ordered[EDGE_TIMESTEPS.index(t)]), (i, t)
    res = _against_fp64(c, table)
    print(f"temb_table unordered {ts}: against fp64 {res}")
    assert res.ratio <= 1.0, res


def test_temb_table_of_all_timesteps():
    """arange(1000) at the shipped layout (half 64, hidden 512, P 1544), as Plan.refresh_weights launches it: row i is bit-equal
    to the row a launch for t = i alone computes, and the whole table is inside the propagated fp64 bound."""
    c = _temb_case(TEMB_LAYOUTS[0], 512, list(range(1000)))
    assert c["wcat"].shape[0] == 1544
    table = _table(c)
    ts = c["t"].to(I32).contiguous()
    alone = torch.full_like(table, NAN)
    ops = _ops()
    for i in range(1000):
        ops.temb_table(ts[i:i + 1], c["freqs"], c["w0"], c["b0"], c["w1"], c["b1"], c["wcat"], c["bcat"], out=alone[i:i + 1])
    assert _same_bits(table, alone)
    res = _against_fp64(c, table)
    TEMB_LINES["shipped/512 x1000"] = (res.ratio, True)
    print(f"temb_table arange(1000): against fp64 {res}")
    assert res.ratio <= 1.0, res


# ---- 3. the one-call step ---------------------------------------------------------------------------------------------------------------------
TINY = dict(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8))
FILL = 0.37109375                   # what every activation buffer holds before a run: finite, exact in fp16
STEP_PLANS = {"fp16-default-64": dict(N=1, dims=(64, 64, 64), dtype=torch.float16, tiny=False),
              "fp16-tiny-b2-odd": dict(N=2, dims=(33, 32, 40), dtype=torch.float16, tiny=True),
              "fp32-tiny-32": dict(N=1, dims=(32, 32, 32), dtype=torch.float32, tiny=True)}
DEFAULT = dict(in_channels=1, out_channels=K.CLASSES, features=K.FEATURES)      # the widths and classes plan_launches is written for


def _make_net(dtype, kw):
    """A DiffUNet with its InstanceNorm affine away from (1, 0): the fused transforms are not identities."""
    from diff_unet_amos_amd.diff_unet import DiffUNet
    torch.manual_seed(0)
    net = DiffUNet(compute_dtype=dtype, **kw)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if ".adn.N." in n:
                p.copy_(torch.randn_like(p) * 0.3 + (1.0 if n.endswith("weight") else 0.0))
    return net.cuda().eval()


@pytest.fixture(scope="module")
def step_plans():
    """name -> (net, plan, staged), built on first use and released when this file is done."""
    cache = {}
    yield lambda name: _step_plan(cache, name)
    cache.clear()
    torch.cuda.empty_cache()


def _step_plan(cache, name):
    """(net, plan, staged): the plan with its weights packed and the condition of one random image resident; ``staged`` holds the
    copies every run starts from."""
    if name not in cache:
        spec = STEP_PLANS[name]
        net = _make_net(spec["dtype"], TINY if spec["tiny"] else DEFAULT)
        assert net.compute_dtype == spec["dtype"]
        N, dims = spec["N"], spec["dims"]
        plan = net._rt.plan(N, dims, torch.device(DEV))
        plan.refresh_weights()
        g = torch.Generator().manual_seed(len(name))
        image = torch.rand(N, 1, *dims, generator=g)
        shape = (N, plan.C, *dims)
        x = torch.randn(*shape, generator=g).to(DEV)
        with torch.no_grad():
            plan.run_encoder(image.to(DEV))
            plan._reset(x)
        staged = dict(xin=plan.xin.clone(), x_state=plan.x_state.clone(), emb=[e.clone() for e in plan.emb],
                      noise=[torch.randn(*shape, generator=g).to(DEV) for _ in range(2)])
        cache[name] = (net, plan, staged)
    return cache[name]


def _buffers(plan):
    named = {"xin": plan.xin, "x4": plan.x4, "den_stats": plan.den_stats, "cur_add": plan.cur_add, "cur_coef": plan.cur_coef,
             "step_word": plan.step_word, "counter": plan.counter, "err_word": plan.err_word, "x_state": plan.x_state, "x_sum": plan.x_sum}
    for key in ("rawA", "rawB", "cat", "pool", "uA", "uB"):
        for l, t in enumerate(getattr(plan, key)):
            named[f"{key}[{l}]"] = t
    return named


def _restage(plan, staged):
    for key in ("rawA", "rawB", "cat", "pool", "uA", "uB"):
        for t in getattr(plan, key):
            t.fill_(FILL)
    plan.x4.fill_(FILL)
    plan.xin.copy_(staged["xin"])
    plan.x_state.copy_(staged["x_state"])
    for e, keep in zip(plan.emb, staged["emb"]):
        e.copy_(keep)
    plan.x_sum.zero_()
    plan.counter.zero_()
    plan.step_word.fill_(-77)
    plan.err_word.zero_()
    plan.cur_add.fill_(FILL)
    plan.cur_coef.fill_(FILL)
    plan.den_stats.fill_(0x0123456789ABCDE)          # the step's own launch must clear it
    plan.seed_word.fill_(20240607)


def _one_step(plan, one_call, mode, rows=None, tables=None, noise=None, logits=None, use_sum=False):
    ops = _ops()
    coef_table, row_of_step = tables if tables is not None else (None, None)
    if one_call:
        plan.native_step(mode, rows_per_sample=rows, row_of_step=row_of_step, coef_table=coef_table, noise=noise, logits=logits,
                         use_sum=use_sum)
        return
    ops.step_begin(plan.N, plan.temb_table, plan.cur_add, rows_per_sample=rows, row_of_step=row_of_step, counter=plan.counter,
                   coef_table=coef_table, cur_coef=plan.cur_coef, step_word=plan.step_word, err_word=plan.err_word, clear=plan.den_stats)
    plan.denoiser_body(zero_stats=False)
    plan.tail(mode, noise=noise, logits=logits, use_sum=use_sum)


def _run(case, kind, one_call):
    """One run from the staged state: snapshots (one per step) of every buffer of the plan and of the outputs."""
    nv = _nv()
    net, plan, staged = case
    _restage(plan, staged)
    snaps = []
    with torch.no_grad():
        if kind == "logits":
            rows = torch.tensor([417, 36][:plan.N], dtype=I32, device=DEV)
            logits = torch.full((plan.N, plan.C, *plan.dims), NAN, dtype=F32, device=DEV)
            _one_step(plan, one_call, nv.MODE_LOGITS, rows=rows, logits=logits)
            snaps.append({**{k: v.clone() for k, v in _buffers(plan).items()}, "logits": logits})
        else:
            tables = plan._step_tables(net.sample_diffusion, kind, 0.0)
            mode = nv.MODE_DDPM if kind == "ddpm" else nv.MODE_DDIM
            for k in range(2):
                _one_step(plan, one_call, mode, tables=tables, noise=staged["noise"][k] if kind == "ddpm" else None, use_sum=kind == "ddim")
                snaps.append({k_: v.clone() for k_, v in _buffers(plan).items()})
    torch.cuda.synchronize()
    return plan, snaps


STEP_CASES = [(name, kind) for name in STEP_PLANS for kind in ("logits", "ddpm", "ddim") if kind == "logits" or name != "fp16-tiny-b2-odd"]


@pytest.mark.parametrize("name,kind", STEP_CASES, ids=[f"{n}-{k}" for n, k in STEP_CASES])
def test_one_call_step_leaves_the_bits_of_the_launch_sequence(step_plans, name, kind):
    """Plan.native_step against ops.step_begin + Plan.denoiser_body(zero_stats=False) + Plan.tail from the same staged state, every
    activation buffer pre-filled with one finite value and the statistics arena with garbage: all buffers, the statistics words,
    cur_add, cur_coef, the device words and the outputs bit for bit (the statistics are integer atomics and every launch is
    reproducible: the expected difference is zero bits)."""
    nv = _nv()
    case = step_plans(name)
    plan, got = _run(case, kind, one_call=True)
    kinds = [o.kind for o in plan._step_ops]
    layout = plan._level0_layout()
    print(f"{name} {kind}: {len(kinds)} recorded ops, kinds {sorted(set(kinds))}, level-0 blocked {layout}")
    if name == "fp16-default-64":
        assert nv.OP_UPCONV in kinds and any(layout) and nv.OP_DECONV in kinds, "the case does not reach what it claims"
    if name == "fp16-tiny-b2-odd":
        assert nv.OP_DECONV_PAD in kinds, "the case does not reach what it claims"
    _, want = _run(case, kind, one_call=False)
    assert len(got) == len(want) == (1 if kind == "logits" else 2)
    for step, (a, b) in enumerate(zip(got, want)):
        diff = [k for k in b if not _same_bits(a[k], b[k])]
        assert not diff, f"{name} {kind} step {step}: the one-call step and the launch sequence differ in {diff}"
        assert int(b["err_word"]) == 0 and bool((b["den_stats"] != 0x0123456789ABCDE).all())
        out = b["logits"] if kind == "logits" else b["x_state"]
        assert bool(torch.isfinite(out).all()) and float(out.std()) > 0
        if kind != "logits":
            assert int(b["counter"]) == step + 1 and int(b["step_word"]) == step
            assert not _same_bits(b["x_state"], case[2]["x_state"])
    if kind == "ddim":
        assert float(want[1]["x_sum"].abs().max()) > 0
    if kind != "logits":
        assert not _same_bits(want[0]["x_state"], want[1]["x_state"])


@pytest.mark.parametrize("case", list(EXPECTED))
def test_recorded_ops_carry_the_pinned_descriptors(case):
    """The OP_CONV3 / OP_DECONV / OP_DECONV_PAD entries of the op list dua_denoiser_step executes carry, field by field and in
    order, the descriptors tests/conv_form_cases.plan_launches writes by hand for the plans of
    tests/test_launch_sequence_fp64.py; the plan hands every convolution the whole split-K workspace."""
    nv, ops = _nv(), _ops()
    from diff_unet_amos_amd.engine import Plan
    exp = EXPECTED[case]
    net = _make_net(torch.float16, DEFAULT)
    N, dims, dt = exp["N"], exp["dims"], exp["dtype"]
    dev = torch.device(DEV)
    plan = net._rt.plan(N, dims, dev) if dt == torch.float16 else Plan(net, N, *dims, torch.float32, dev)
    plan.refresh_weights()
    assert [plan._fold_level(l) for l in range(4)] == exp["fold"] and plan._level0_layout() == exp["layout"]
    logits = torch.zeros((N, plan.C, *dims), dtype=F32, device=dev)
    with torch.no_grad():
        plan.native_step(nv.MODE_LOGITS, rows_per_sample=torch.tensor(TIMESTEPS[:N], dtype=I32, device=dev), logits=logits)
    torch.cuda.synchronize()
    assert int(plan.err_word) == 0
    recorded = list(plan._step_ops)
    assert len(recorded) == len(exp["seq"]) - 1
    assert sum(o.kind == nv.OP_UPCONV for o in recorded) == sum(exp["fold"]) and sum(o.kind == nv.OP_MATERIALIZE for o in recorded) == 5
    convs = [o for o in recorded if o.kind in (nv.OP_CONV3, nv.OP_DECONV, nv.OP_DECONV_PAD)]
    launches = K.plan_launches(case, exp)
    assert len(convs) == len(launches)
    p = plan._step_keep[0]
    ws_bytes = plan.splitk_ws.numel() * plan.splitk_ws.element_size()
    assert p.workspace == plan.splitk_ws.data_ptr() and p.workspace_bytes == ws_bytes and p.n_ops == len(recorded)
    deconv_policy = 6 if (ops.CONV_POLICY & 0xff) == 6 else 0
    for o, (name, kind, d, fused, out_dims) in zip(convs, launches):
        got = tuple(getattr(o.conv, f) for f in K.FIELDS)
        if kind == "conv":
            assert o.kind == nv.OP_CONV3, name
            assert got == K.with_fields(d, policy=ops.CONV_POLICY), (case, name, dict(zip(K.FIELDS, got)))
            assert ops.conv3_form(o.conv, fused, ws_bytes).workspace_needed <= ws_bytes, (case, name)
        else:
            padded = tuple(out_dims) != tuple(2 * e for e in d[2:5])
            assert o.kind == (nv.OP_DECONV_PAD if padded else nv.OP_DECONV), name
            assert got == K.with_fields(d, policy=deconv_policy), (case, name, dict(zip(K.FIELDS, got)))
            if padded:
                assert (o.mat.D, o.mat.H, o.mat.W) == tuple(out_dims), (case, name)
        assert o.has_norm == (1 if fused else 0), (case, name)


# ---- 4. bad arguments, next to launches that succeed ------------------------------------------------------------------------------------------
def _resolver(valid):
    """NULL -> the null pointer; ODD -> the valid argument's own address 4 bytes on (4-byte aligned, inside the same buffer)."""
    return lambda name, marker: None if marker == SR.NULL else C.c_void_p(valid[name].value + 4)


@pytest.mark.parametrize("mode", ["rows", "steps"])
def test_step_begin_rejects_bad_arguments_and_writes_nothing(mode):
    """step_ref.BEGIN_BAD on real tensors: the valid argument set launches (return 0, the expected row copy, the arena cleared);
    the same set with one bad argument returns ERR_ARG and leaves every output, device word, guard and the arena as they were."""
    nv = _nv()
    lib, E = nv.lib(), nv.ERR_ARG
    stepped = mode == "steps"
    s = _Begin(2, 257, 5 if stepped else 0, _row_of_step(5, None) if stepped else None)
    buf, arena = _guarded(64, 3.5, lead=4)
    rows = None if stepped else torch.tensor([3, 0], dtype=I32, device=DEV)
    valid = dict(N=s.N, P=s.P, table=nv.ptr(s.table), table_rows=TABLE_ROWS, rows_per_sample=nv.ptr(rows), row_of_step=nv.ptr(s.ros),
                 nsteps=s.nsteps, coef_table=nv.ptr(s.coef), counter=nv.ptr(s.counter), cur_add=nv.ptr(s.cur_add), cur_coef=nv.ptr(s.cur_coef),
                 step_word=nv.ptr(s.step_word), err_word=nv.ptr(s.err_word), clear=nv.ptr(arena), clear_bytes=4 * arena.numel())
    s.expect(rows_per_sample=None if stepped else [3, 0])
    assert SR.call_step_begin_clear(lib, valid, nv.stream_ptr()) == 0
    s.check(f"{mode}: the valid call")
    assert bool((arena.view(I32) == 0).all()) and _guards_intact(buf, arena)
    arena.fill_(3.5)
    taken = 0
    for applies, bad in SR.BEGIN_BAD:
        if applies == "steps" and not stepped:
            continue
        assert SR.call_step_begin_clear(lib, SR.with_bad(valid, bad, _resolver(valid)), nv.stream_ptr()) == E, (mode, bad)
        s.check(f"{mode}: {bad}")
        assert bool((arena == 3.5).all()) and _guards_intact(buf, arena), (mode, bad)
        taken += 1
    assert taken == (17 if stepped else 13)


def test_temb_table_rejects_bad_arguments_and_writes_nothing():
    """step_ref.TABLE_BAD on real tensors: the valid call returns 0 and writes the table ops.temb_table writes; one bad argument
    returns ERR_ARG and leaves the NaN-filled table as it was."""
    nv = _nv()
    lib, E = nv.lib(), nv.ERR_ARG
    c = _temb_case(TEMB_LAYOUTS[4], 256, EDGE_TIMESTEPS)
    want = _table(c)
    ts = c["t"].to(I32).contiguous()
    T, P = want.shape
    buf, out = _guarded(T * P)
    valid = dict(count=T, timesteps=nv.ptr(ts), freqs=nv.ptr(c["freqs"]), half=c["half"], hid=c["hid"], w0=nv.ptr(c["w0"]), b0=nv.ptr(c["b0"]),
                 w1=nv.ptr(c["w1"]), b1=nv.ptr(c["b1"]), wcat=nv.ptr(c["wcat"]), bcat=nv.ptr(c["bcat"]), P=P, table=nv.ptr(out))
    assert SR.call_temb_table(lib, valid, nv.stream_ptr()) == 0
    assert _same_bits(out.view(T, P), want) and _guards_intact(buf, out)
    out.fill_(NAN)
    for bad in SR.TABLE_BAD:
        assert SR.call_temb_table(lib, SR.with_bad(valid, bad, _resolver(valid)), nv.stream_ptr()) == E, bad
        assert bool(torch.isnan(out).all()) and _guards_intact(buf, out), bad


STEP_BAD = [dict(N=0), dict(N=-1), dict(ops=None), dict(n_ops=0), dict(n_ops=-1), dict(stat_arena=None), dict(stat_bytes=0),
            dict(stat_bytes=-16), dict(tail_raw=None)]


def test_denoiser_step_first_line_rejects_and_launches_nothing(step_plans):
    """The struct of a step that has just run (Plan._step_keep), copied with one field made bad: ERR_ARG, and every buffer of the
    restaged plan -- cur_add, the statistics arena full of garbage, the device words, all activations -- keeps its bits.  Every
    other field is valid, so nothing behind the first line of dua_denoiser_step can be what answers for ``ops``, ``n_ops``,
    ``stat_bytes = 0`` and ``tail_raw``: without that line the step (or its step_begin launch) would run and the buffers change.
    N <= 0, a NULL arena and stat_bytes < 0 are refused a second time by dua_step_begin_clear before its launch; no caller can
    tell the two lines apart for those, they are listed for completeness."""
    nv = _nv()
    case = step_plans("fp32-tiny-32")
    plan, snaps = _run(case, "logits", one_call=True)               # the positive control: the unmodified struct runs
    assert int(snaps[0]["err_word"]) == 0 and bool(torch.isfinite(snaps[0]["logits"]).all())
    good = plan._step_keep[0]
    _restage(plan, case[2])
    before = {k: v.clone() for k, v in _buffers(plan).items()}
    for bad in STEP_BAD:
        p = nv.DenoiserPlan.from_buffer_copy(good)
        for k, v in bad.items():
            setattr(p, k, C.POINTER(nv.StepOp)() if k == "ops" else v)
        assert nv.lib().dua_denoiser_step(C.byref(p), nv.stream_ptr()) == nv.ERR_ARG, bad
        torch.cuda.synchronize()
        diff = [k for k, v in _buffers(plan).items() if not _same_bits(v, before[k])]
        assert not diff, f"{bad}: the call changed {diff}"
