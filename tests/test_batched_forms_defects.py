"""The checks of tests/test_batched_forms_fp64.py can fail: on the inputs of every case there, the fp64 reference is built once as
it is and once with one batch mix-up planted -- another sample's scale / shift / add rows, the D-face halo read from the sample
next in memory instead of zeros, one split-K partial taken from sample n + 1 -- and the two differ by more than the derived bound.
A kernel that made the mistake would land within its bound of the tampered reference; the tampered reference is required to lie
more than TWICE the bound away from the true one on at least one element, so such a kernel cannot pass.  No GPU: the InstanceNorm
constants come from fp64 sums of the raw tensor (the GPU tests hold the preamble's own values to these).

Evaluated at the voxels where the defects act and a few inside: both D faces of every sample, three planes in between."""
import pytest
import torch

import batched_form_cases as B
import fp64ref as R

MARGIN = 2.0


def _voxels(N, dims):
    """[P, 4]: per sample the planes d = 0, 1, D / 2, D - 1 at a 3 x 3 lattice of (h, w) that touches every H and W face"""
    D, H, W = dims
    return torch.tensor([(n, d, h, w) for n in range(N) for d in sorted({0, 1, D // 2, D - 1})
                         for h in (0, H // 2, H - 1) for w in (0, W // 2, W - 1)], dtype=torch.int64)


def _ratio(ref, mixed, bnd):
    return float(((mixed - ref).abs() / bnd).max())


def test_the_whole_volume_references_equal_the_gathered_ones():
    """conv3_sums / fold_sums (shifted products over a padded tensor) against fp64ref.gather_taps + conv3_ref / fold_parents +
    fold_ref (a gather per point) at every voxel of a small ragged volume: the same three sums to fp64 rounding."""
    g = torch.Generator().manual_seed(5)
    N, dims, cin, cout = 2, (4, 6, 2), 8, 5
    x = torch.randn(N, *dims, cin, generator=g).half()
    w, b = torch.randn(cout, cin, 3, 3, 3, generator=g), torch.randn(cout, generator=g)
    Wm = R.conv3_weights(w, B.F16)
    pts = R.all_voxels(N, dims)
    A, _ = R.gather_taps(x, pts, 0, cin)
    for got, want in zip(B.conv3_sums(B.padded(x.double()), Wm, b), R.conv3_ref(A, Wm, b)):
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)
    sel = pts[::3]
    for got, want in zip(B.conv3_sums(B.padded(x.double()), Wm, b, sel), R.conv3_ref(A[::3], Wm, b)):
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)
    cu, cmid = 64, 8
    u = torch.randn(N, *(s // 2 for s in dims), cu, generator=g).double()
    wc, wd = torch.randn(cout, cin + cmid, 3, 3, 3, generator=g), torch.randn(cu, cmid, 2, 2, 2, generator=g)
    bc, bd = torch.randn(cout, generator=g), torch.randn(cmid, generator=g)
    Wp = {k: m for k, (m, _) in R.compose_fold(wc[:, cin:], wd).items()}
    rows, arows = R.fold_bias_table(wc[:, cin:], bc, bd)
    Ws = R.conv3_weights(wc[:, :cin], B.F16)
    par, ok, phi, deltas = R.fold_parents(pts, dims)
    pc = torch.minimum(par.clamp_min(0), torch.tensor([s // 2 - 1 for s in dims]))
    U = u[pts[:, None, 0].expand_as(ok), pc[..., 0], pc[..., 1], pc[..., 2]]
    cls = R.border_class(pts, dims)
    want = R.fold_ref(A, Ws, U, ok, phi, deltas, Wp, rows[cls], arows[cls])
    got = B.fold_sums(B.conv3_sums(B.padded(x.double()), Ws), dims, u, Wp, rows, arows)
    for a, b_ in zip(got[:3], want):
        assert torch.allclose(a.reshape(-1, cout), b_, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", list(B.CONV_CASES))
def test_a_planted_batch_mix_up_exceeds_the_bound(name):
    N, dims, cin, cout, fused, (kernel, depth, ksplit), grid = B.CONV_CASES[name]
    assert N >= 2 and grid[2] == N * ksplit
    t = B.conv_inputs(name)
    consts = B.host_consts(t["x"], t["gamma"], t["beta"], t["add"]) if fused else None
    if fused:                                                    # the rows of neighbouring samples are far apart to begin with
        sc, sh, ad = consts
        for n in range(N):
            m = (n + 1) % N
            assert float(((sc[n] - sc[m]).abs() / sc[n].abs()).median()) > 0.1 and float((ad[n] - ad[m]).abs().median()) > 0.1
    Wm = R.conv3_weights(t["w"], B.F16)
    sel = _voxels(N, dims)
    act = B.activation(t["x"], consts)
    ref, ab, sq = B.conv3_sums(B.padded(act), Wm, t["b"], sel)
    bnd = B.conv_bound(ref, ab, sq, cin, fused, ksplit)
    found = {}
    if fused:
        rows = [(n + 1) % N for n in range(N)]
        mixed = B.conv3_sums(B.padded(B.activation(t["x"], consts, rows)), Wm, t["b"], sel)[0]
        found["rows of sample n + 1"] = _ratio(ref, mixed, bnd)
        # each kind of row on its own: a kernel may index one of them wrongly and the others rightly
        for k, what in enumerate(("scale", "shift", "add")):
            c = [v[rows] if j == k else v for j, v in enumerate(consts)]
            mixed = B.conv3_sums(B.padded(B.activation(t["x"], c)), Wm, t["b"], sel)[0]
            found[f"{what} row of sample n + 1"] = _ratio(ref, mixed, bnd)
    mixed = B.conv3_sums(B.padded(act, d_halo_from_neighbours=True), Wm, t["b"], sel)[0]
    on_face = (sel[:, 1] == 0) | (sel[:, 1] == dims[0] - 1)
    assert torch.equal(mixed[~on_face], ref[~on_face])           # the defect acts on the D faces only
    found["D-face halo from the neighbouring sample"] = _ratio(ref, mixed, bnd)
    if ksplit > 1:
        ups = -(-3 * -(-cin // 32) // ksplit)
        assert ksplit * ups >= 3 * -(-cin // 32) > (ksplit - 1) * ups
        other = B.padded(torch.roll(act, -1, 0)) - B.padded(act)
        for part in range(ksplit):
            keep = B.split_rows(cin, ups, part)
            assert int(keep.sum()) == 9 * 32 * ups
            Wj = torch.where(keep[:, None], Wm, torch.zeros_like(Wm))
            mixed = ref + B.conv3_sums(other, Wj, None, sel)[0]
            found[f"split-K partial {part} of sample n + 1"] = _ratio(ref, mixed, bnd)
    print(f"\n{name}: max |tampered - true| / bound at {len(sel)} voxels x {cout} channels")
    for what, r in found.items():
        print(f"  {what:<44} {r:12.1f}")
    weak = {k: r for k, r in found.items() if not r > MARGIN}
    assert not weak, f"{name}: the inputs do not tell these mix-ups from rounding: {weak}"


def test_a_planted_mix_up_of_the_fold_s_rows_exceeds_the_bound():
    """The folded up-convolution of FOLD_CASE with the coarse tensor's scale / shift / add rows of sample n + 1; composed weights as
    the packer forms them (fp64 composition, one rounding)."""
    N, dims, cskip, cu, cmid, cout = B.FOLD_CASE
    t = B.fold_inputs()
    consts = B.host_consts(t["u"], t["gamma"], t["beta"], t["add"])
    Wp = {k: m.half().double() for k, (m, _) in R.compose_fold(t["wc"][:, cskip:], t["wd"]).items()}
    rows, arows = R.fold_bias_table(t["wc"][:, cskip:], t["bc"], t["bd"])
    Wm = R.conv3_weights(t["wc"][:, :cskip], B.F16)
    keep = slice(0, 2)                                           # two samples are enough to tell them apart, and quicker
    skip_sums = B.conv3_sums(B.padded(t["skip"][keep].double()), Wm)

    def fold(u_act):
        return B.fold_sums(skip_sums, dims, u_act[keep], Wp, rows, arows)

    act = B.activation(t["u"], consts)
    ref, ab, sq, ar = fold(act)
    bnd = R.bound(ref, ab, sq, R.chain_length(27 * cskip + 8 * cu, B.F16), B.F16, emulated_in=B.F16, extra=R.U32 * (27 * cmid + 1) * ar)
    found = {"rows of sample n + 1": _ratio(ref, fold(B.activation(t["u"], consts, [(n + 1) % N for n in range(N)]))[0], bnd)}
    print(f"\nfold {N}x{dims} {cskip}+{cu}->{cout}: max |tampered - true| / bound over 2 samples: {found}")
    assert all(r > MARGIN for r in found.values()), found
