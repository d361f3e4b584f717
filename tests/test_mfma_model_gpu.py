"""The premise of every fp64 check of an MFMA kernel, on the instruction itself: dua_mfma_single issues ONE v_mfma_f32_32x32x16_f16 or
v_mfma_f32_16x16x32_f16 per tile (D = C + A . B, one wave), and D is compared with the exact sum formed in integers
(tests/mfma_model.py: the operand sets, the model, what the sweeps showed).  Every element of every set must lie within the model at
the width fp64ref.MFMA_W; the measured alignment widths are printed per class and must not fall below MFMA_W + 1 (the constant keeps
one guard bit).  tests/test_mfma_model_ref.py shows without a device that these sets reject a window two bits narrower and flushed
subnormal inputs."""
import numpy as np
import pytest
import torch

import fp64ref as R
import mfma_model as MM

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _run(shape_code, A, B, C):
    from diff_unet_amos_amd import _native as nv
    a, b, c = (torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in (A, B, C))
    d = torch.full_like(c, float("nan"))
    nv.check(nv.lib().dua_mfma_single(shape_code, A.shape[0], nv.ptr(a), nv.ptr(b), nv.ptr(c), nv.ptr(d), nv.stream_ptr()), "dua_mfma_single")
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("shape", list(MM.SHAPES))
def test_operand_layout_of_the_probe(shape):
    """Small integers: exact in any arithmetic, so D == C + A B^T pins the lane maps of the entry point itself."""
    code, MN, K = MM.SHAPES[shape]
    g = np.random.default_rng(0)
    A, B = (g.integers(-8, 9, (3, MN, K)).astype(np.float16) for _ in range(2))
    C = g.integers(-8, 9, (3, MN, MN)).astype(np.float32)
    D = _run(code, A, B, C)
    assert np.array_equal(D, C + np.einsum("tik,tjk->tij", A.astype(np.float64), B.astype(np.float64)))


@pytest.mark.parametrize("shape", list(MM.SHAPES))
def test_window_sweeps_within_the_model(shape):
    code, MN, K = MM.SHAPES[shape]
    a, b, c, rec = MM.sweep_cases(K)
    At, Bt, Ct, idx = MM.diagonal_tiles(a, b, c, MN)
    D = _run(code, At, Bt, Ct).reshape(-1)[idx]
    widths = MM.measured_widths(D, a, b, c, rec)
    for (cls, form, when), (good, lost) in sorted(widths.items()):
        print(f"{shape} small product {cls}, {form}, {when}: exact down to {good} places below the largest nominal exponent, "
              f"first loss at {lost}")
    measured = MM.alignment_width(widths)
    print(f"{shape}: measured alignment width {measured}; fp64ref.MFMA_W = {R.MFMA_W}")
    r = MM.ratios(D, a, b, c, R.MFMA_W)
    k = int(r.argmax())
    print(f"{shape}: {r.size} sweep cases, worst |D - exact| / model {r[k]:.3f} (j={rec['j'][k]} class={MM.SMALL_CLASSES[rec['cls'][k]]} "
          f"form={MM.C_MODES[rec['form'][k]]} k={rec['k'][k]} p={rec['p'][k]})")
    assert r.max() <= 1.0, (shape, float(r[k]), {n: int(v[k]) for n, v in rec.items()})
    assert measured >= R.MFMA_W + 1, (shape, measured)
    # a product added after the large terms have cancelled meets nothing that could push it out of the window
    assert all(lost is None for (_, _, when), (_, lost) in widths.items() if when == "after-cancel"), widths


@pytest.mark.parametrize("name", list(MM.RANDOM_SETS))
@pytest.mark.parametrize("shape", list(MM.SHAPES))
def test_random_operands_within_the_model(shape, name):
    """Exponent fields over the whole fp16 range (or its low end, or subnormals only), zeros, both signs, C from far below to far above
    the products; every element of every tile."""
    code, MN, K = MM.SHAPES[shape]
    A, B, C = MM.random_set(shape, name)
    D = _run(code, A, B, C)
    a, b, c = MM.tile_rows(A, B, C)
    sub = lambda v: float(((v != 0) & (np.abs(v.astype(np.float64)) < 2.0 ** -14)).mean())      # noqa: E731
    r = MM.ratios(D.reshape(-1), a, b, c, R.MFMA_W)
    print(f"{shape} {name}: {r.size} elements, subnormal share of A {sub(A):.2f} / B {sub(B):.2f}, worst |D - exact| / model {r.max():.3f}")
    assert r.max() <= 1.0, (shape, name, float(r.max()), int(r.argmax()))
