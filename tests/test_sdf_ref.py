"""The contract of dua_sdf_maps on the CPU (tests/sdf_ref.py): the exhaustive restatement against scipy's squared distances stored
in tests/golden/sdf_golden.npz, the fp32 form against Kervadec's fp64 formula within the derived bound, every planted defect of the
emulation caught on a (shape, kind) the GPU test runs, and the argument checks of the C entries (no device needed)."""
import ctypes as C
import os

import numpy as np
import pytest

import sdf_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdf_golden.npz")
CASES = [(si, kind) for si in range(len(R.SHAPES)) for kind in R.KINDS]


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def contracts():
    """(labels, phi, d2) of every case, computed once."""
    out = {}
    for si, kind in CASES:
        y = R.make_labels(R.SHAPES[si], kind)
        out[si, kind] = (y,) + R.contract(y)
    return out


def test_the_golden_file_holds_every_case_and_stays_small(golden):
    """Well under the size of components_golden.npz, the largest of the label-geometry goldens: at most three quarters of it."""
    assert os.path.getsize(GOLDEN) <= 0.75 * os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "components_golden.npz"))
    assert sorted(golden) == sorted(CASES)


def test_the_restatement_equals_scipys_squared_distances(golden, contracts):
    for si, kind in CASES:
        y, _, d2 = contracts[si, kind]
        pos = y > np.float32(0.5)
        bits, want = golden[si, kind]
        assert np.array_equal(np.packbits(pos.reshape(-1)), bits), (si, kind)       # the generator is stable
        assert want.dtype == np.int32 and d2.dtype == np.int32 and np.array_equal(d2, want), (R.SHAPES[si], kind)


def test_all_pairs_and_per_axis_search_agree():
    """brute_d2 takes all pairs where it can afford them and the exhaustive per-axis minimum elsewhere: the same integers."""
    for kind in ("random30", "box3", "soft"):
        pos = R.make_labels(R.SHAPES[0], kind)[0, 0] > np.float32(0.5)
        d2 = R.brute_d2(pos)
        sep = np.where(pos, R._separable_d2(~pos), R._separable_d2(pos))
        assert np.array_equal(d2, sep), kind


def test_the_fp32_contract_is_within_the_bound_of_the_fp64_formula(contracts):
    worst = 0.0
    for (si, kind), (y, phi, d2) in contracts.items():
        pos = y > np.float32(0.5)
        assert phi.dtype == np.float32
        ratio = np.abs(phi.astype(np.float64) - R.fp64_formula(d2, pos)) / R.bound(d2)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (R.SHAPES[si], kind, float(ratio.max()))
    print(f"worst |phi_fp32 - phi_fp64| / bound: {worst:.3f}")
    assert worst > 0.1          # the bound is not slack by an order of magnitude


def test_the_rules_of_the_contract(contracts):
    """absent / full volumes are 0 throughout; 0.5 itself is outside, the next float inside; inside values are <= 0."""
    for si in range(len(R.SHAPES)):
        for kind in ("absent", "full"):
            _, phi, d2 = contracts[si, kind]
            assert not phi.any() and not d2.any()
        y, phi, d2 = contracts[si, "soft"]
        assert (y == np.float32(0.5)).any() and (y == R.HALF_UP).any()
        assert (phi[y == np.float32(0.5)] >= 1).all() and (phi[y == R.HALF_UP] <= 0).all()
        assert (d2 >= 1).all()


def test_the_emulation_without_a_defect_is_the_contract(contracts):
    for (si, kind), (y, phi, d2) in contracts.items():
        e_phi, e_d2 = R.emulate(y)
        assert np.array_equal(e_d2, d2) and np.array_equal(e_phi.view(np.int32), phi.view(np.int32)), (R.SHAPES[si], kind)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect, contracts):
    """On at least one (shape, kind) of the GPU test's list the defective emulation differs from the contract in phi or d2 -- the
    comparison the GPU test makes -- so that test cannot pass over such a kernel."""
    caught = []
    for (si, kind), (y, phi, d2) in contracts.items():
        e_phi, e_d2 = R.emulate(y, defect=defect)
        if not (np.array_equal(e_phi.view(np.int32), phi.view(np.int32)) and np.array_equal(e_d2, d2)):
            caught.append((R.SHAPES[si], kind))
    print(defect, "caught on", len(caught), "cases, e.g.", caught[:3])
    assert caught, defect
    if defect == "d2_16bit":                            # only the two shapes with an extent of 512 reach d2 >= 2^16
        assert {s for s, _ in caught} == {R.SHAPES[5], R.SHAPES[6]}


def test_the_c_entries_refuse_bad_arguments_without_a_device():
    from diff_unet_amos_amd import _native as nv
    lib = nv.lib()
    one = C.c_void_p(16)
    big = 1 << 40
    assert lib.dua_sdf_scratch_bytes(2, 3, 5, 7, 9) == 2 * 3 * 5 * 7 * 9 * 4
    assert lib.dua_sdf_scratch_bytes(1, 1, 512, 512, 512) == 512 ** 3 * 4
    for bad in ((0, 1, 4, 4, 4), (1, 0, 4, 4, 4), (1, 1, 0, 4, 4), (1, 1, 4, 513, 4), (1, 1, 4, 4, 513), (256, 256, 4, 4, 4)):
        assert lib.dua_sdf_scratch_bytes(*bad) == nv.ERR_ARG, bad
        assert lib.dua_sdf_maps(*bad, one, 0.5, one, None, one, big, None) == nv.ERR_ARG, bad
    ok = (1, 2, 4, 5, 6)
    need = lib.dua_sdf_scratch_bytes(*ok)
    assert lib.dua_sdf_maps(*ok, None, 0.5, one, None, one, need, None) == nv.ERR_ARG          # no labels
    assert lib.dua_sdf_maps(*ok, one, 0.5, None, None, one, need, None) == nv.ERR_ARG          # no phi
    assert lib.dua_sdf_maps(*ok, one, 0.5, one, None, None, need, None) == nv.ERR_ARG          # no scratch
    assert lib.dua_sdf_maps(*ok, one, 0.5, one, None, one, need - 1, None) == nv.ERR_ARG       # scratch too small
    assert lib.dua_sdf_maps(*ok, one, float("nan"), one, None, one, need, None) == nv.ERR_ARG  # a NaN threshold
