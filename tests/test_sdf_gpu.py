"""dua_sdf_maps on the GPU (csrc/sdf.hip through ops.signed_distance_maps) against the numpy restatement of its contract
(tests/sdf_ref.py): phi and d2 bit for bit on every shape and label kind -- at 96^3 too, where lines are longer than a wave and
tiles are full -- two runs equal, a captured replay equal to the eager
call, and the aliasing rule (phi may be written over the labels)."""
import numpy as np
import pytest
import torch

import sdf_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(shape, kind) for shape in R.SHAPES for kind in R.KINDS] + [(R.BIG_SHAPE, kind) for kind in R.BIG_KINDS]
_REF = {}


def _case(shape, kind):
    """(labels on the device, phi, d2 of the restatement as CPU tensors), computed once per case and never modified."""
    if (shape, kind) not in _REF:
        y = R.make_labels(shape, kind)
        phi, d2 = R.contract(y)
        _REF[shape, kind] = (torch.from_numpy(y).to(DEV), torch.from_numpy(phi), torch.from_numpy(d2))
    return _REF[shape, kind]


def _bits(x):
    return x.view(torch.int32)


@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in CASES])
def test_phi_and_d2_equal_the_restatement(shape, kind):
    from diff_unet_amos_amd import ops
    y, phi, d2 = _case(shape, kind)
    got_d2 = torch.full(shape, -7, dtype=torch.int32, device=DEV)
    got = ops.signed_distance_maps(y, d2=got_d2)
    again = ops.signed_distance_maps(y)                                  # no d2 asked for: the same phi
    torch.cuda.synchronize()
    assert torch.equal(got_d2.cpu(), d2), (shape, kind, int((got_d2.cpu() != d2).sum()))
    assert torch.equal(_bits(got.cpu()), _bits(phi)), (shape, kind)      # bits: -0.0 would not pass for 0.0
    assert torch.equal(_bits(again), _bits(got))


def test_another_threshold_and_the_strict_comparison():
    from diff_unet_amos_amd import ops
    y, _, _ = _case(R.SHAPES[0], "soft")
    for t in (0.25, 0.75, float(R.HALF_UP)):
        phi, d2 = R.contract(y.cpu().numpy(), t)
        got_d2 = torch.empty(R.SHAPES[0], dtype=torch.int32, device=DEV)
        got = ops.signed_distance_maps(y, threshold=t, d2=got_d2)
        assert torch.equal(got_d2.cpu(), torch.from_numpy(d2)) and torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(phi))), t


def test_a_captured_replay_equals_the_eager_call():
    from diff_unet_amos_amd import ops
    shape = R.SHAPES[4]
    y, phi, d2 = _case(shape, "partition")
    buf = torch.zeros_like(y)
    out, od2 = torch.empty_like(y), torch.empty(shape, dtype=torch.int32, device=DEV)
    scratch = torch.empty(y.numel(), dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.signed_distance_maps(buf, out=out, d2=od2, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.signed_distance_maps(buf, out=out, d2=od2, scratch=scratch)
    for kind in ("partition", "random30"):                               # new labels reach the replay through the input buffer
        y, phi, d2 = _case(shape, kind)
        buf.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(od2.cpu(), d2) and torch.equal(_bits(out.cpu()), _bits(phi)), kind


def test_phi_may_be_written_over_the_labels_and_d2_may_alias_nothing():
    """The labels are consumed by the first pass (include/dua_hip.h): out=labels is allowed and gives the same bits; d2 aliasing
    an operand is refused."""
    from diff_unet_amos_amd import ops
    shape = R.SHAPES[3]
    y, phi, d2 = _case(shape, "random30")
    work = y.clone()
    got = ops.signed_distance_maps(work, out=work)
    assert got.data_ptr() == work.data_ptr() and torch.equal(_bits(work.cpu()), _bits(phi))
    with pytest.raises(AssertionError):
        ops.signed_distance_maps(y, d2=y.view(torch.int32))
    room = torch.empty(2 * y.numel(), dtype=torch.int32, device=DEV)
    half = y.numel() // 2
    with pytest.raises(AssertionError):                                  # a partial overlap is an overlap
        ops.signed_distance_maps(y, out=room[:y.numel()].view(torch.float32).view(shape), d2=room[half:half + y.numel()].view(shape))
    with pytest.raises(AssertionError):
        ops.signed_distance_maps(y, out=room[:y.numel()].view(torch.float32).view(shape), scratch=room[half:half + y.numel()])
    assert torch.equal(y.cpu(), torch.from_numpy(R.make_labels(shape, "random30")))          # the shared case is untouched


def test_extents_outside_the_limits_are_refused():
    from diff_unet_amos_amd import ops
    with pytest.raises(AssertionError):
        ops.signed_distance_maps(torch.zeros(1, 1, 1, 1, 513, device=DEV))
    with pytest.raises(AssertionError):
        ops.signed_distance_maps(torch.zeros(1, 1, 4, 4, 4, device=DEV).half())
