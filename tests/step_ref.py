"""References of the sampler step's own kernels (csrc/temb.hip: step_begin_kernel, temb_table_kernel), in the style of
tests/glue_fp64ref.py.  A plain helper module (``import step_ref``); tests/test_step_ref.py tests it on the CPU,
tests/test_step_gpu.py holds the kernels to it.

step_begin is exact.  ``step_begin_ref`` is plain torch indexing with the kernel's clamp as the contract: an index below 0 reads
entry 0, an index at or above the length reads the last entry, either case raises the error word (nothing else writes it).  The
step index is the counter (clamped to [0, nsteps - 1]) or, with ``rows_per_sample``, k = 0: the coefficient row every sample then
receives is row 0 of the table, and neither the counter nor the step word is touched.

temb_table against float64.  ``temb_table_ref`` is the chained float64 evaluation of the embedder (glue_fp64ref.temb_fwd_ref
with ``saved=None``: every stage on the reference's own previous stage) and a bound of |table - ref| per element.  The kernel's
arithmetic per output row is that of temb_train_fwd (arg = fl((float) t freq); a lane-strided fmaf chain from 0; the 32..1 xor
tree; one add of the bias; x (1 / (1 + expf(-x)))), so the stage bounds are glue_fp64ref's (u = 2^-24, sin / cos 4 ulp, exp
3 ulp; derivation there).  Those bound one stage on the input its launch READ; here nothing of the device's is read, so the
error of a stage's input is carried to its output by first-order worst case:

    e    : b_e  = 4 ulp |e| + DEN                                                  (no earlier error: arg is an exact operand)
    z1   : b_z1 = rows(W0, e, b0; 8 u sum |w e|)                                   (glue_fp64ref._rows carries b_e itself)
    h1   : b_h1 = L(z1, b_z1) b_z1 + swish-bound(z1)
    z2   : b_z2 = |W1| b_h1 + rows(W1, h1, b1)
    s    : b_s  = L(z2, b_z2) b_z2 + swish-bound(z2)
    add  : b    = |Wcat| b_s + rows(Wcat, s, bcat)

    rows(W, x, b) = (ceil(K / 64) + 7) u (sum |w x| + |b|)      L(z, b) = min(1.1, |swish'(z)| + b / 2) >= sup |swish'| on [z - b, z + b]

swish'(x) = s + x s (1 - s) lies in [-0.0998, 1.0998] (|swish'| <= 1.1 everywhere) and |swish''| = |s (1 - s) (2 + x (1 - 2 s))| <= 1/2
(its maximum, at 0), hence L.  |W| b_x is the worst case of W (x' - x) for |x' - x| <= b_x.  The rounding terms are evaluated at
the reference's stage values, not at the device's: the difference is a product of two relative errors of <= 1e-4 each, and the
whole bound is multiplied by SECOND_ORDER (as every first-order sum of glue_fp64ref is).  No number comes from a device run.

How loose it is.  Worst-case propagation through a K-wide row adds K magnitudes that in fact carry independent signs: through
the two 512-wide layers that alone is roughly sqrt(K) ~ 20x per layer, and the 4 ulp granted to sinf / cosf (the device library
is far inside it) is multiplied through both; observed errors sit about three orders of magnitude below the bound (DESIGN.md
section 10h).  This check guards against a
defect that the table kernel and its training twin share; the tight check is the bit-equality of the two kernels' outputs
(tests/test_step_gpu.py), with the training forward held stage by stage to glue_fp64ref.  So that the worst-case bound cannot
hide a failure, ``bound_is_tight_enough`` requires bound <= 0.05 (|ref| + rms of ref over the row) on >= 99 % of a table's entries.

``emu_temb_table`` restates temb_table_kernel's own order of operations in torch fp32 on the CPU, with the planted defects
tests/test_step_ref.py rejects.
"""
from __future__ import annotations

import torch

import glue_fp64ref as GR

F32, F64 = torch.float32, torch.float64
SWISH_SLOPE = 1.1             # sup |swish'| over the reals is 1.0998
SWISH_CURVE = 0.5             # sup |swish''| (at 0)
CAP_FRACTION, CAP_SHARE = 0.05, 0.99


# ---- step_begin ---------------------------------------------------------------------------------------------------------------------
def _clamp(i, n):
    """(clamped index, whether it was outside [0, n))"""
    i = int(i)
    return min(max(i, 0), n - 1), not 0 <= i < n


def step_begin_ref(N, table, rows_per_sample=None, row_of_step=None, counter=None, coef_table=None):
    """What one step_begin launch leaves: dict(cur_add [N, P], cur_coef [N, 8] or None (no ``coef_table``), step_word and counter
    (ints; None with ``rows_per_sample``: untouched), err (True: the launch raises the error word; False: it leaves it alone)).
    ``table`` [rows, P], ``rows_per_sample`` / ``row_of_step`` integer sequences or tensors, ``counter`` the value before the
    launch, ``coef_table`` [nsteps, 8] (with ``rows_per_sample``: at least one row)."""
    rows_n = table.shape[0]
    bad, k = False, 0
    if rows_per_sample is None:
        nsteps = len(row_of_step)
        k, bad = _clamp(counter, nsteps)
        picks = [row_of_step[k]] * N
    else:
        assert len(rows_per_sample) == N
        picks = list(rows_per_sample)
    idx = []
    for r in picks:
        r, off = _clamp(r, rows_n)
        bad = bad or off
        idx.append(r)
    cur_add = table[torch.tensor(idx, dtype=torch.int64, device=table.device)]
    cur_coef = None
    if coef_table is not None:
        cur_coef = coef_table.reshape(-1, 8)[k].expand(N, 8).clone()
    stepped = rows_per_sample is None
    return dict(cur_add=cur_add, cur_coef=cur_coef, step_word=k if stepped else None, counter=k + 1 if stepped else None, err=bad)


# ---- temb_table -----------------------------------------------------------------------------------------------------------------------
def _dswish(x):
    s, om = torch.sigmoid(x), torch.sigmoid(-x)
    return s + x * s * om


def _swish_carried(z, b_z):
    """(swish(z), bound of the device's swish of its own z within b_z of ``z``)"""
    ref, rounding = GR.swish_ref(z)
    slope = torch.clamp(_dswish(z.double()).abs() + SWISH_CURVE * b_z, max=SWISH_SLOPE)
    return ref, slope * b_z + rounding


def _rows_carried(W, x, b_x, bias, extra_u=0.0):
    ref, rounding = GR._rows(W, x, bias, extra_u=extra_u)
    return ref, b_x @ W.double().abs().t() + rounding


def temb_table_ref(t, freqs, w0, b0, w1, b1, wcat, bcat):
    """(ref, bound), float64 [T, P]: row i = wcat swish(W1 swish(W0 [sin | cos](t_i freqs) + b0) + b1) + bcat and the bound of the
    table kernel's row against it (module docstring).  ``t``: integer timesteps [T], any order, repeats allowed."""
    chained = GR.temb_fwd_ref(t.to(torch.int64), freqs, w0, b0, w1, b1, [wcat], [bcat], saved=None)
    e = chained["e"][0]
    z1, b_z1 = GR._rows(w0, e, b0, extra_u=GR.SINCOS_ULPS * GR.ULP)
    h1, b_h1 = _swish_carried(z1, b_z1)
    z2, b_z2 = _rows_carried(w1, h1, b_h1, b1)
    s, b_s = _swish_carried(z2, b_z2)
    ref, bound = _rows_carried(wcat, s, b_s, bcat)
    assert torch.equal(ref.reshape(-1), chained["add"][0]), "the carried chain and glue_fp64ref.temb_fwd_ref are one evaluation"
    return ref, bound * GR.SECOND_ORDER


def bound_share_within_cap(ref, bound):
    """Share of the entries with bound <= CAP_FRACTION (|ref| + rms of ref over the row)."""
    rms = ref.pow(2).mean(1, keepdim=True).sqrt()
    return float((bound <= CAP_FRACTION * (ref.abs() + rms)).double().mean())


def bound_is_tight_enough(ref, bound):
    return bound_share_within_cap(ref, bound) >= CAP_SHARE


def _emu_rows(W, x, bias, drop_last_stride=False, stride=None):
    """One matrix-vector stage of temb_table_kernel: lane l chains fmaf over k = l, l + 64, ..; the xor tree; the bias.
    ``stride``: distance between the rows of ``W`` in memory (default K); ``drop_last_stride``: the planted defect."""
    R, K = W.shape
    if stride is not None and stride != K:
        flat = GR._f(W).reshape(-1)
        at = (torch.arange(R)[:, None] * stride + torch.arange(K)[None, :]).clamp_max(flat.numel() - 1)
        W = flat[at]
    n = GR._cdiv(K, 64)
    Wp = torch.nn.functional.pad(GR._f(W), (0, n * 64 - K)).view(R, n, 64)
    xp = torch.nn.functional.pad(GR._f(x), (0, n * 64 - K)).view(-1, n, 64)
    acc = torch.zeros(xp.shape[0], R, 64, dtype=F32)
    for i in range(n - 1 if drop_last_stride and K % 64 else n):
        acc = GR._fma(Wp[None, :, i], xp[:, None, i], acc)
    return GR._f(GR._wave_tree(acc) + GR._f(bias))


DEFECTS = ("last_stride", "no_second_swish", "bcat_twice", "wcat_stride")


def emu_temb_table(t, freqs, w0, b0, w1, b1, wcat, bcat, defect=None):
    """temb_table_kernel in torch fp32 on the CPU (a correctly rounded library function stands in for sinf / cosf / expf):
    [T, P].  ``defect``: last_stride (the last lane stride of a row dropped where K is no multiple of 64), no_second_swish,
    bcat_twice, wcat_stride (row o of wcat read at o (hid - 1))."""
    assert defect is None or defect in DEFECTS
    hid = w1.shape[0]
    arg = GR._f(t.to(F32)[:, None] * GR._f(freqs)[None, :])
    e = torch.cat([GR._f(torch.sin(arg.double())), GR._f(torch.cos(arg.double()))], 1)
    last = defect == "last_stride"
    h1 = GR.emu_swish(_emu_rows(w0, e, b0, drop_last_stride=last))
    z2 = _emu_rows(w1, h1, b1, drop_last_stride=last)
    h2 = z2 if defect == "no_second_swish" else GR.emu_swish(z2)
    out = _emu_rows(wcat, h2, bcat, drop_last_stride=last, stride=hid - 1 if defect == "wcat_stride" else None)
    return GR._f(out + GR._f(bcat)) if defect == "bcat_twice" else out


# ---- layouts shared by the CPU and the GPU file ---------------------------------------------------------------------------------------
def swin_widths(feature_size):
    """Output widths of the fifteen t_proj of the Swin plan in table order (swin_engine.SwinPlan._bind: swinViT.t_proj[0..4], the
    residual blocks encoder1, 2, 3, 4, 10, decoder1..5)."""
    f = feature_size
    return [f, 2 * f, 4 * f, 8 * f, 16 * f] + [f, f, 2 * f, 4 * f, 16 * f] + [f, f, 2 * f, 4 * f, 8 * f]


def swin_blocks(feature_size):
    """[(width, is_pad)] of the table columns as swin_engine.refresh_weights lays them out: every projection's rows, then all-zero
    rows (zero bias) up to the next multiple of 8 -- each padded run a block of its own."""
    out = []
    for c in swin_widths(feature_size):
        out.append((c, False))
        if -c % 8:
            out.append((-c % 8, True))
    return out


def make_layout_params(hid, half, blocks, seed, device="cpu"):
    """glue_fp64ref.make_temb_params over ``blocks`` (widths, or (width, is_pad) pairs: a pad block's weights and bias are zero)."""
    blocks = [(b, False) if isinstance(b, int) else b for b in blocks]
    w0, b0, w1, b1, ws, bs = GR.make_temb_params(hid, half, [c for c, _ in blocks], seed, device)
    for (_, pad), w, b in zip(blocks, ws, bs):
        if pad:
            w.zero_()
            b.zero_()
    return w0, b0, w1, b1, ws, bs


def pad_mask(blocks):
    """bool [P]: the table columns that belong to a pad block."""
    blocks = [(b, False) if isinstance(b, int) else b for b in blocks]
    return torch.cat([torch.full((c,), bool(pad)) for c, pad in blocks])


def rows_of_block_major(flat, N, couts):
    """The block-major ``add`` of temb_train_fwd as table rows [N, P]."""
    return torch.cat(GR.block_rows(flat, N, couts), 1)


# ---- bad arguments, shared by the CPU file (made-up addresses, nothing valid is ever called) and the GPU file (real tensors, next to a
# ---- launch that succeeds) -----------------------------------------------------------------------------------------------------------------
NULL, ODD = "null", "odd"           # markers a test resolves: the NULL pointer; the argument's own pointer 4 bytes further (misaligned)
BEGIN_ARGS = ("N", "P", "table", "table_rows", "rows_per_sample", "row_of_step", "nsteps", "coef_table", "counter", "cur_add", "cur_coef",
              "step_word", "err_word", "clear", "clear_bytes")
TABLE_ARGS = ("count", "timesteps", "freqs", "half", "hid", "w0", "b0", "w1", "b1", "wcat", "bcat", "P", "table")
# one bad argument each: every DUA_ERR_ARG branch of dua_step_begin_clear.  The valid call they are applied to has a coefficient
# table with its cur_coef and a 16-byte aligned arena of a multiple of 16 bytes; "steps" cases apply without rows_per_sample only.
BEGIN_BAD = [("any", kw) for kw in (dict(N=0), dict(N=-1), dict(P=0), dict(P=-8), dict(table=NULL), dict(table_rows=0), dict(table_rows=-1),
                                    dict(cur_add=NULL), dict(cur_coef=NULL), dict(clear_bytes=-16), dict(clear_bytes=24), dict(clear=NULL),
                                    dict(clear=ODD))]
BEGIN_BAD += [("steps", kw) for kw in (dict(row_of_step=NULL), dict(counter=NULL), dict(nsteps=0), dict(nsteps=-1))]
TABLE_BAD = [dict(count=0), dict(count=-1), dict(half=0), dict(half=-1), dict(hid=0), dict(hid=-256), dict(P=0), dict(P=-1)]
TABLE_BAD += [{name: NULL} for name in ("timesteps", "freqs", "w0", "b0", "w1", "b1", "wcat", "bcat", "table")]


def with_bad(valid, bad, resolve):
    """``valid`` (name -> argument) with the overrides of ``bad``; ``resolve(name, marker)`` turns NULL / ODD into a pointer."""
    return {**valid, **{k: resolve(k, v) if v in (NULL, ODD) else v for k, v in bad.items()}}


def call_step_begin_clear(lib, args, stream=None):
    return lib.dua_step_begin_clear(*[args[k] for k in BEGIN_ARGS], stream)


def call_temb_table(lib, args, stream=None):
    return lib.dua_temb_table(*[args[k] for k in TABLE_ARGS], stream)
