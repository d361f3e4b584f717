"""tests/step_ref.py on the CPU: the indexing reference of step_begin against hand-written expectations for every clamp case; the
float64 reference of temb_table against the embedder restated with torch.nn.functional, its propagated bound against torch fp32
emulations of the kernels' own operation order (inside) and against four planted defects (outside), and the cap that keeps the
worst-case bound from hiding a failure, for every layout tests/test_step_gpu.py runs.  The last tests need only the shared
library: every argument check of dua_step_begin_clear and dua_temb_table, and the NULL plan of dua_denoiser_step, answer before
anything is launched (on made-up addresses; tests/test_step_gpu.py repeats the cases on real tensors next to valid launches)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import glue_fp64ref as GR
import step_ref as SR
from test_glue_fp64 import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
EDGE_TIMESTEPS = [0, 1, 2, 499, 998, 999]
SWIN = [("swin48", 64, SR.swin_blocks(48)), ("swin12", 64, SR.swin_blocks(12))]
ALL_LAYOUTS = [(n, h, [(c, False) for c in couts]) for n, h, couts in LAYOUTS] + SWIN


# ---- step_begin_ref --------------------------------------------------------------------------------------------------------------------
def _table(rows, P):
    return (torch.arange(rows * P, dtype=F32).view(rows, P) + 0.5)


def _coefs(nsteps):
    return -(torch.arange(nsteps * 8, dtype=F32).view(nsteps, 8) + 1)


def test_step_begin_ref_rows_per_sample():
    tab, coef = _table(5, 3), _coefs(4)
    r = SR.step_begin_ref(3, tab, rows_per_sample=[4, 0, 4], coef_table=coef)
    assert r["cur_add"].tolist() == [[12.5, 13.5, 14.5], [0.5, 1.5, 2.5], [12.5, 13.5, 14.5]]
    assert r["cur_coef"].tolist() == [[-1, -2, -3, -4, -5, -6, -7, -8]] * 3          # k = 0: row 0 for every sample
    assert r["step_word"] is None and r["counter"] is None and r["err"] is False
    r = SR.step_begin_ref(1, tab, rows_per_sample=torch.tensor([2], dtype=torch.int32))
    assert r["cur_add"].tolist() == [[6.5, 7.5, 8.5]] and r["cur_coef"] is None and r["err"] is False


@pytest.mark.parametrize("rows,want,err", [([-1, 1], [0, 1], True), ([1, 5], [1, 4], True), ([-1, 5], [0, 4], True), ([0, 4], [0, 4], False)])
def test_step_begin_ref_clamps_a_row(rows, want, err):
    tab = _table(5, 3)
    r = SR.step_begin_ref(2, tab, rows_per_sample=rows)
    assert torch.equal(r["cur_add"], tab[want]) and r["err"] is err


@pytest.mark.parametrize("counter,k,err", [(0, 0, False), (3, 3, False), (4, 3, True), (-1, 0, True), (7, 3, True)])
def test_step_begin_ref_counter(counter, k, err):
    tab, coef, ros = _table(5, 3), _coefs(4), [4, 2, 2, 0]
    r = SR.step_begin_ref(2, tab, row_of_step=ros, counter=counter, coef_table=coef)
    assert torch.equal(r["cur_add"], tab[[ros[k]] * 2]) and torch.equal(r["cur_coef"], coef[[k, k]])
    assert (r["step_word"], r["counter"], r["err"]) == (k, k + 1, err)


def test_step_begin_ref_counter_and_row_clamps_are_independent():
    tab = _table(5, 3)
    r = SR.step_begin_ref(1, tab, row_of_step=[1, -1, 5], counter=1)
    assert torch.equal(r["cur_add"], tab[[0]]) and (r["step_word"], r["counter"], r["err"], r["cur_coef"]) == (1, 2, True, None)
    r = SR.step_begin_ref(1, tab, row_of_step=[1, -1, 5], counter=2)
    assert torch.equal(r["cur_add"], tab[[4]]) and (r["counter"], r["err"]) == (3, True)
    r = SR.step_begin_ref(1, tab, row_of_step=[1, -1, 5], counter=3)             # both: the last step's row, itself off the table
    assert torch.equal(r["cur_add"], tab[[4]]) and (r["step_word"], r["counter"], r["err"]) == (2, 3, True)
    r = SR.step_begin_ref(1, tab, row_of_step=[1, -1, 5], counter=0)
    assert torch.equal(r["cur_add"], tab[[1]]) and r["err"] is False


def test_step_begin_ref_single_step_and_single_row():
    tab = _table(1, 4)
    for counter, err in ((0, False), (1, True), (-1, True)):
        r = SR.step_begin_ref(2, tab, row_of_step=[0], counter=counter, coef_table=_coefs(1))
        assert torch.equal(r["cur_add"], tab[[0, 0]]) and (r["step_word"], r["counter"], r["err"]) == (0, 1, err)


# ---- temb_table_ref ----------------------------------------------------------------------------------------------------------------------
def _case(layout, hid, timesteps, seed=3):
    name, half, blocks = layout
    w0, b0, w1, b1, ws, bs = SR.make_layout_params(hid, half, blocks, seed)
    t = torch.tensor(timesteps, dtype=torch.int64)
    return dict(t=t, freqs=GR.temb_freqs(half), w0=w0, b0=b0, w1=w1, b1=b1, ws=ws, bs=bs, wcat=torch.cat(ws, 0), bcat=torch.cat(bs, 0),
                couts=[w.shape[0] for w in ws])


def _table_args(c):
    return c["t"], c["freqs"], c["w0"], c["b0"], c["w1"], c["b1"], c["wcat"], c["bcat"]


def _layout(name):
    return next(l for l in ALL_LAYOUTS if l[0] == name)


def test_temb_table_ref_is_the_embedder():
    """float64 through torch.nn.functional, written from the model's definition: sinusoid [sin | cos], Linear, swish, Linear, the
    swish every block applies, the concatenated projections."""
    lin = torch.nn.functional.linear
    c = _case(_layout("shipped"), 512, EDGE_TIMESTEPS + [37])
    ref, bound = SR.temb_table_ref(*_table_args(c))
    arg = (c["t"].float()[:, None] * c["freqs"][None, :]).double()
    e = torch.cat([arg.sin(), arg.cos()], 1)
    assert torch.equal(e[0], torch.cat([torch.zeros(64), torch.ones(64)]).double())         # t = 0: e = [0 | 1]
    h = torch.nn.functional.silu(lin(e, c["w0"].double(), c["b0"].double()))
    h = torch.nn.functional.silu(lin(h, c["w1"].double(), c["b1"].double()))
    want = lin(h, c["wcat"].double(), c["bcat"].double())
    assert ref.shape == (7, 1544) and float((ref - want).abs().max()) < 1e-12
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())


@pytest.mark.parametrize("name,hid", [("shipped", 512), ("ragged145", 256), ("half3", 256), ("swin12", 512)])
def test_bound_accepts_the_kernels_own_arithmetic(name, hid):
    """The training forward's emulation re-laid out to rows, and the table kernel's (one row chain each: bit-equal on the CPU as
    the kernels are expected to be on the device), inside the propagated bound."""
    c = _case(_layout(name), hid, EDGE_TIMESTEPS + [417, 1])
    ref, bound = SR.temb_table_ref(*_table_args(c))
    add, _ = GR.emu_temb_fwd(c["t"], c["freqs"], c["w0"], c["b0"], c["w1"], c["b1"], c["ws"], c["bs"])
    twin = SR.rows_of_block_major(add, c["t"].numel(), c["couts"])
    table = SR.emu_temb_table(*_table_args(c))
    assert torch.equal(table, twin)
    res = GR.check(table, ref, bound)
    print(f"{name} hid {hid}: emulation {res}")
    assert res.ratio <= 1.0, res
    assert torch.equal(table[1], table[-1])                                                # t = 1 twice: the same row
    pads = SR.pad_mask(_layout(name)[2])
    assert bool((table[:, pads] == 0).all()) and bool((ref[:, pads] == 0).all())


@pytest.mark.parametrize("defect,name,hid", [("last_stride", "half3", 256), ("last_stride", "half3", 512), ("no_second_swish", "shipped", 512),
                                             ("bcat_twice", "shipped", 512), ("wcat_stride", "shipped", 512),
                                             ("no_second_swish", "P129", 256), ("bcat_twice", "P129", 256), ("wcat_stride", "P129", 256)])
def test_bound_rejects_planted_defects(defect, name, hid):
    c = _case(_layout(name), hid, EDGE_TIMESTEPS)
    ref, bound = SR.temb_table_ref(*_table_args(c))
    ok = GR.check(SR.emu_temb_table(*_table_args(c)), ref, bound)
    bad = GR.check(SR.emu_temb_table(*_table_args(c), defect=defect), ref, bound)
    print(f"{defect} at {name} hid {hid}: {bad.ratio:.3g} (intact {ok.ratio:.3g})")
    assert ok.ratio <= 1.0 and bad.ratio > 1.0, (ok, bad)


@pytest.mark.parametrize("hid", [256, 512])
@pytest.mark.parametrize("layout", ALL_LAYOUTS, ids=[l[0] for l in ALL_LAYOUTS])
def test_bound_cannot_hide_a_failure(layout, hid):
    """At least 99 % of the entries of every table the device test checks have bound <= 0.05 (|ref| + rms of the row): from the
    operands alone, with the parameters and timesteps of the device test (tests/test_step_gpu.py uses the same seed)."""
    c = _case(layout, hid, EDGE_TIMESTEPS)
    ref, bound = SR.temb_table_ref(*_table_args(c))
    share = SR.bound_share_within_cap(ref, bound)
    print(f"{layout[0]} hid {hid}: {100 * share:.2f} % of the entries within the cap, median bound / |ref| "
          f"{float((bound / ref.abs().clamp_min(1e-30)).median()):.2e}")
    assert SR.bound_is_tight_enough(ref, bound), share


# ---- argument errors: no device needed ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from diff_unet_amos_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "diff_unet_amos_amd", "csrc"), "-j4"], check=True)
    return _native.lib()


def test_step_entry_points_reject_bad_arguments_without_a_device(lib):
    """Every call below carries exactly one bad argument (step_ref.BEGIN_BAD / TABLE_BAD, applied to made-up addresses) and must
    return ERR_ARG before anything is launched.  The valid argument sets themselves cannot be called without a device:
    tests/test_step_gpu.py applies the same lists to real tensors next to launches that succeed, and takes the first line of
    dua_denoiser_step there too (behind that line dua_step_begin_clear would answer ERR_ARG for a made-up plan as well, so here
    only the NULL plan is told apart)."""
    from diff_unet_amos_amd import _native as nv
    E = nv.ERR_ARG
    one = C.c_void_p(256)                                  # a 16-byte aligned non-null address

    def resolve(name, marker):
        return None if marker == SR.NULL else C.c_void_p(260)

    rows_mode = dict(N=2, P=8, table=one, table_rows=4, rows_per_sample=one, row_of_step=None, nsteps=0, coef_table=one, counter=None,
                     cur_add=one, cur_coef=one, step_word=None, err_word=None, clear=one, clear_bytes=32)
    steps_mode = dict(rows_mode, rows_per_sample=None, row_of_step=one, nsteps=3, counter=one)
    taken = 0
    for mode, bad in SR.BEGIN_BAD:
        for valid in ([rows_mode] if mode == "any" else []) + [steps_mode]:
            assert SR.call_step_begin_clear(lib, SR.with_bad(valid, bad, resolve)) == E, (mode, bad)
            taken += 1
    assert taken == 2 * 13 + 4
    assert lib.dua_step_begin(0, 8, one, 4, one, None, 0, None, None, one, None, None, None, None) == E
    table = dict(count=3, timesteps=one, freqs=one, half=4, hid=256, w0=one, b0=one, w1=one, b1=one, wcat=one, bcat=one, P=8, table=one)
    for bad in SR.TABLE_BAD:
        assert SR.call_temb_table(lib, SR.with_bad(table, bad, resolve)) == E, bad
    assert len(SR.TABLE_BAD) == 8 + 9
    assert lib.dua_denoiser_step(None, None) == E
