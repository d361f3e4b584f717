"""The sampler tail's fp64 references and bounds (tests/sampler_fp64ref.py) on the CPU: the update reference equals the oracle's
p_sample / ddim_sample in float64 on every row of both schedules; the Philox restatement reproduces the Random123 known-answer
vectors; a torch fp32 emulation of the kernel's own arithmetic is inside every bound on the inputs of every case of
tests/test_sampler_fp64.py (reduced voxel counts); each of ten planted defects is outside one (ratio > 1, so a test fails if its
mutation is removed); and the inputs exercise both sides of the clamp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import fp64ref as R
import sampler_fp64ref as T
from oracle.diffusion_ref import RefDiffusion

VOX = 600                  # reduced voxel count of the host runs: more than two 256-voxel tiles, a partial last one
MODES = (T.DDPM, T.DDIM)


# ---- the update reference against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [10, 1000])
@pytest.mark.parametrize("eta", [0.0, 0.3, 1.0])
def test_update_ref_equals_the_oracle_on_every_row(steps, eta):
    """oracle.diffusion_ref.RefDiffusion in float64 on the same logits: the oracle gathers its float64 tables and casts them to
    fp32 (GD:904-917), as the package's coefficient rows do."""
    rd = RefDiffusion(1000, [steps])
    g = torch.Generator().manual_seed(steps)
    t = torch.arange(steps)
    shape = (steps, 3, 2, 2, 5)
    L = 1.5 * torch.randn(shape, generator=g, dtype=torch.float64)
    xt, eps = torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)
    fn = lambda x, tt, **kw: L
    ts = [(steps, int(i)) for i in t]
    view = lambda rows: rows.view(steps, 1, 1, 1, 1, 8)
    if eta == 0.0:                                  # the DDPM step has no eta: checked once per schedule
        want = rd.p_sample(fn, xt, t, eps)
        x0, xn, _, _ = T.update_ref(T.DDPM, view(T.coef_rows(ts, T.DDPM)), L, xt, eps)
        assert torch.equal(x0, want["pred_xstart"])
        assert float((xn - want["sample"]).abs().max()) <= 1e-12 * float(want["sample"].abs().max())
    want = rd.ddim_sample(fn, xt, t, eps, eta=eta)
    x0, xn, _, _ = T.update_ref(T.DDIM, view(T.coef_rows(ts, T.DDIM, eta)), L, xt, eps)
    assert torch.equal(x0, want["pred_xstart"])
    # the oracle forms sqrt(acp_prev) etc. from fp32 tables in fp32; the rows from float64 tables rounded once: 2^-23 relative
    tol = 4 * 2.0 ** -23 * (1 + 1 / float(T.coef_rows(ts, T.DDIM, eta)[:, 1].abs().min()))
    assert float((xn - want["sample"]).abs().max()) <= tol * float(want["sample"].abs().max()), eta


# ---- the noise generator ------------------------------------------------------------------------------------------------------
KAT = [  # Random123 kat_vectors, philox4x32-10: counter, key, result
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_restatement_reproduces_the_known_answer_vectors(ctr, key, want):
    got = T.philox4x32_10(np.array(ctr, dtype=np.uint64), *key)
    assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


def test_philox_normals_layout_and_moments():
    """counter = (lo32(gv), hi32(gv), step, quad) with gv = n vox + v, key = (lo32(seed), hi32(seed)): sample 1 of a batch is
    the continuation of sample 0's voxels, each term changes the field, and the field is standard normal."""
    a = T.philox_normals(T.SEED64, T.STEP, 2, 700, 4)
    b = T.philox_normals(T.SEED64, T.STEP, 1, 1400, 4)
    assert a.shape == (2, 700, 16) and np.array_equal(a.reshape(1400, 16), b[0])
    assert np.array_equal(T.philox_normals(T.SEED64, T.STEP, 1, 64, 8)[..., :16], b[:, :64])
    for other in (T.philox_normals(T.SEED64 & 0xFFFFFFFF, T.STEP, 1, 1400, 4), T.philox_normals(T.SEED64, T.STEP + 1, 1, 1400, 4)):
        assert abs(float((other * b).mean())) < 0.03 and not np.array_equal(other, b)
    big = T.philox_normals(T.SEED64, T.STEP, 1, 40000, 4)
    assert abs(big.mean()) < 1e-2 and abs(big.std() - 1) < 1e-2 and abs((big ** 4).mean() - 3) < 0.1
    # a voxel index beyond 2^32 reaches the counter's second word
    w = T.philox4x32_10(np.array([[5, 1, 7, 0], [5, 0, 7, 0]], dtype=np.uint64), 1, 2)
    assert not np.array_equal(w[0], w[1])


# ---- the emulation inside the bounds, the planted defects outside --------------------------------------------------------------
_CACHE = {}


def _case(name, use_ra=True):
    key = (name, use_ra)
    if key not in _CACHE:
        c = T.build_case(name, VOX)
        c["use_ra"] = use_ra
        consts = ()
        if c["form"] != "identity":
            consts = T.host_constants(c["raw"], c["gamma"], c["beta"])
        if c["form"] == "res":
            consts = consts + T.host_constants(c["res"], c["rgamma"], c["rbeta"])
        quads = c["cx"] // 4
        eps = torch.from_numpy(T.philox_normals(T.SEED64, T.STEP, c["N"], VOX, quads)).float()    # an fp32 field, as the kernel holds it
        _CACHE[key] = (c, consts, eps)
    return _CACHE[key]


RUNS = [(n, True) for n in T.CASES] + [("d1", False), ("d2", False)]


@pytest.mark.parametrize("name,use_ra", RUNS, ids=[f"{n}{'' if r else '-no-ra'}" for n, r in RUNS])
@pytest.mark.parametrize("mode", MODES)
def test_emulation_within_bounds_and_every_defect_outside(name, use_ra, mode):
    c, consts, eps = _case(name, use_ra)
    ref = T.case_reference(c, consts, mode, eps.double())
    inside, below, above = T.input_conditions(ref["L"])
    print(f"\ncase {name} {mode}: logits inside (-1, 1) {inside:.3f}, below -1 {below:.3f}, above 1 {above:.3f}, "
          f"std {float(ref['L'].std()):.3f}")
    assert inside >= 0.40 and below >= 0.05 and above >= 0.05
    ratio, where = T.worst_ratio(T.emulate_tail(c, consts, mode, eps), ref)
    print(f"  honest emulation: {ratio:.4f} ({where})")
    assert ratio <= 1.0, where
    for m in T.MUTATIONS:
        if m in T.SPLIT_MUTATIONS and c["form"] == "valu":
            continue                                  # the VALU form has no fp16 pairs to lose
        if m in ("drop_aw_yl", "act_fp16_only") and c["form"] == "identity":
            continue                                  # the identity form's activation is an fp16 value: its lo half is 0
        r, w = T.worst_ratio(T.emulate_tail(c, consts, mode, eps, mutate=m), ref)
        print(f"  {m:<16} {r:12.4g}")
        assert r > 1.0, (m, w)


def test_grid_and_tile_walk_of_the_cases():
    """The walks the GPU file asserts, for the 256 CUs they are stated for."""
    for name, c in T.CASES.items():
        if "wgs" not in c:
            continue
        V = c["dims"][0] * c["dims"][1] * c["dims"][2]
        w = T.tile_walk(V, c["N"], c["wgs"], 256)
        assert (w["tiles"], w["g"], w["walks"], w["last"]) == (c["tiles"], c["g"], c["walks"], c["last"]), (name, w)
        assert w["walks"][0] >= 2                     # every persistent case loops


# ---- the VALU form's LDS limit ---------------------------------------------------------------------------------------------------
def test_valu_tail_refuses_what_its_lds_cannot_hold():
    """(CX + 3) K floats of dynamic LDS without a raised limit: CX = 32 with K > 464 is DUA_ERR_ARG before any launch (host side,
    no device: the refusal comes before the first HIP call); K = 464 and CX = 24 at K = 512 pass the argument checks of the
    descriptor (they are not launched here)."""
    from diff_unet_amos_amd import _native as nv
    if not os.path.exists(nv.LIB_PATH):
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        subprocess.run(["make", "-C", os.path.join(root, "diff_unet_amos_amd", "csrc"), "-j4"], check=True)
    lib = nv.lib()
    one = C.c_void_p(16)

    def call(dtype, K, Cc, CX):
        d = nv.TailDesc(dtype, 1, 1000, K, K, Cc, CX, nv.MODE_DDPM, 0, 0, None)
        return lib.dua_final_conv_sampler(C.byref(d), one, None, one, one, one, one, one, None, None, None, None, None, None)

    for dtype in (nv.F32, nv.F16):
        for K in (472, 480, 512):
            assert call(dtype, K, 29, 32) == nv.ERR_ARG, (dtype, K)
    assert (32 + 3) * 464 * 4 <= 65536 < (32 + 3) * 472 * 4 and (24 + 3) * 512 * 4 <= 65536
