"""The AMOS loss set (cfg/amos/train.yaml: losses mse,bce,multi_neighbor,dice, loss_combine sum): the multi_neighbor term of
losses/loss.py:234-301 on the HIP kernels (csrc/multi_neighbor.hip) and through the fused loss and the trainers.

The CPU restatement below is checked against tests/golden/multi_neighbor_golden.npz, which the reference's own
MultiNeighborLoss produced (tools/make_multi_neighbor_golden.py); the kernels are checked against the restatement."""
import os

import numpy as np
import pytest
import torch

from oracle.train_ref import RefLoss, ref_training_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "multi_neighbor_golden.npz")
AMOS = "mse,bce,multi_neighbor,dice"


# ---- restatement (CPU, fp32) -------------------------------------------------------------------------------------------------
def _class_centroids(vol, K):
    """vol [C, D, H, W]: every (c, h, w) column votes for the depth of its maximum (torch.argmax over dim 1: first maximum,
    NaN wins); class k's centroid is the mean (c, h, w) of the columns that voted k.  Returns (centroids [K, 3] fp32, present
    [K] bool); absent classes keep (0, 0, 0)."""
    vote = vol.argmax(dim=1).reshape(-1)
    C, H, W = vol.shape[0], vol.shape[2], vol.shape[3]
    coords = torch.stack(torch.meshgrid(torch.arange(C), torch.arange(H), torch.arange(W), indexing="ij"), -1)
    coords = coords.reshape(-1, 3).float()
    centroids = torch.zeros(K, 3)
    present = torch.zeros(K, dtype=torch.bool)
    for k in range(K):
        hit = vote == k
        if bool(hit.any()):
            centroids[k] = coords[hit].mean(0)
            present[k] = True
    return centroids, present


def _pair_angles(cent):
    """Angles between the unit differences u[a][b] and u[a][e] for b < e (a, b, e over the rows of cent)."""
    v = cent[:, None, :] - cent[None, :, :]
    length = v.norm(dim=-1, keepdim=True)
    length = torch.where(length > 0, length, torch.ones_like(length))
    u = v / (length + 1e-6)
    cos = torch.matmul(u, u.transpose(1, 2)).clamp(-1 + 1e-6, 1 - 1e-6)
    m = len(cent)
    b, e = torch.triu_indices(m, m, 1)
    return torch.acos(cos)[:, b, e].reshape(-1)


def multi_neighbor_restated(logits, labels, K):
    """losses/loss.py:234-301 in other words.  logits [N, C, D, H, W] (any float dtype; the sigmoid is taken in fp32),
    labels [N, C, D, H, W]; fp32 result."""
    deltas = []
    for i in range(logits.shape[0]):
        lc, valid = _class_centroids(labels[i].float(), K)
        pc, _ = _class_centroids(torch.sigmoid(logits[i].float()), K)
        if int(valid.sum()) < 2:
            deltas.append(torch.zeros(1))
            continue
        deltas.append((_pair_angles(pc[valid]) - _pair_angles(lc[valid])) ** 2)
    return torch.cat(deltas).mean()


def labels_from_classes(classes, C):
    cl = torch.as_tensor(classes).long()
    onehot = torch.nn.functional.one_hot(cl.clamp(min=0), C).permute(0, 4, 1, 2, 3).float()
    return (onehot * (cl >= 0).unsqueeze(1).float()).contiguous()


def _golden_cases():
    g = np.load(GOLDEN)
    names = sorted({k.rsplit("_", 1)[0] for k in g.files if k.endswith("_value")})
    return [(n, torch.from_numpy(g[f"{n}_logits"]), labels_from_classes(g[f"{n}_classes"], g[f"{n}_logits"].shape[1]),
             int(g[f"{n}_K"]), float(g[f"{n}_value"])) for n in names]


def _amos_criterion(combine):
    """losses/loss.py:64-86 over mse, bce, multi_neighbor, dice: the oracle's three terms plus the restated one (no grad)."""
    three = RefLoss("mse,bce,dice", "sum").losses

    def crit(preds, labels):
        mse, bce, dice = (f(torch.sigmoid(preds), labels) if isinstance(f, torch.nn.MSELoss) else f(preds, labels) for f in three)
        mn = multi_neighbor_restated(preds.detach(), labels, preds.shape[1]).to(preds.dtype)
        terms = torch.stack([mse, bce, mn, dice])
        if combine == "sum":
            return terms.sum()
        if combine == "mean":
            return terms.mean()
        return torch.log(1 + terms.sum())
    return crit


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_parse_losses_accepts_the_amos_set():
    from diff_unet_amos_amd.training import parse_losses
    assert parse_losses(AMOS, "sum") == (("mse", "bce", "multi_neighbor", "dice"), "sum")
    assert parse_losses("multi_neighbor,dice", "log") == (("multi_neighbor", "dice"), "log")
    assert parse_losses("dice,mse,multi_neighbor", "mean") == (("dice", "mse", "multi_neighbor"), "mean")


@pytest.mark.parametrize("names", ["mse,bce,multi_neighbor,focal", "hausdorff_er", "multi_neighbour"])
def test_other_names_are_still_refused(names):
    from diff_unet_amos_amd.training import parse_losses
    bad = [n for n in names.split(",") if n not in ("mse", "bce", "dice", "multi_neighbor")][0]
    with pytest.raises(NotImplementedError, match=rf"Loss \({bad}\) is not listed yet"):
        parse_losses(names, "sum")


def test_gradient_names_are_unchanged():
    from diff_unet_amos_amd import ops
    assert ops.LOSS_NAMES == ("mse", "bce", "dice")
    assert set(ops.SEG_LOSS_NAMES) == {"mse", "bce", "dice", "multi_neighbor"}


def test_restatement_equals_the_reference_golden():
    cases = _golden_cases()
    assert {c[0] for c in cases} == {"noncubic", "saturated", "k_lt_c"}
    for name, logits, labels, K, want in cases:
        got = float(multi_neighbor_restated(logits, labels, K))
        assert abs(got - want) <= 1e-6 * abs(want), (name, got, want)


def test_restatement_pins_the_depth_argmax_and_the_saturation_tie():
    """The class of a column is the depth of its maximum; saturated logits tie at sigmoid 1.0 and the first depth wins."""
    logits = torch.full((1, 2, 5, 1, 2), -4.0)
    logits[0, :, 1] = 20.0
    logits[0, :, 3] = 31.0                   # larger logit, same fp32 sigmoid (1.0): depth 1 wins, not 3
    vote = torch.sigmoid(logits[0]).argmax(dim=1)
    assert vote.eq(1).all()
    labels = torch.zeros(1, 2, 5, 1, 2)
    labels[0, 0, 3, 0, 0] = 1.0
    labels[0, 1, 2, 0, 1] = 1.0
    _, valid = _class_centroids(labels[0], 5)
    assert valid.tolist() == [True, False, True, True, False]      # the unlabelled columns vote 0


def test_trainer_refuses_multi_neighbor_alone():
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    net = DiffUNet(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8))
    with pytest.raises(ValueError, match="no gradient"):
        NativeConvTrainer(net, losses="multi_neighbor")


def test_new_entry_points_reject_bad_arguments():
    """The C ABI's multi_neighbor entry points validate before any launch (no device needed)."""
    import ctypes as C
    from diff_unet_amos_amd import _native as nv
    L, one = nv.lib(), C.c_void_p(16)
    assert L.dua_multi_neighbor_columns(nv.F16, 1, 16, 65, 8, 8, 8, one, 16, one, one, None) == nv.ERR_ARG    # K > 64
    assert L.dua_multi_neighbor_columns(nv.F16, 1, 16, 16, 8, 8, 8, one, 8, one, one, None) == nv.ERR_ARG    # stride < C
    assert L.dua_multi_neighbor_columns(7, 1, 16, 16, 8, 8, 8, one, 16, one, one, None) == nv.ERR_ARG         # dtype
    assert L.dua_multi_neighbor_columns(nv.F32, 1, 16, 16, 0, 8, 8, one, 16, one, one, None) == nv.ERR_ARG    # empty extent
    assert L.dua_multi_neighbor_angles(1, 0, one, one, None) == nv.ERR_ARG
    assert L.dua_multi_neighbor_angles(1, 16, None, one, None) == nv.ERR_ARG
    assert L.dua_seg_loss_finish_mn(1, 4, 10, 1, 0, 0, 4, None, 0, one, one, one, None) == nv.ERR_ARG          # no partials
    assert L.dua_seg_loss_finish_mn(1, 4, 10, 1, 0, 0, 4, one, 0, None, one, one, None) == nv.ERR_ARG          # mse, no sums
    assert L.dua_seg_loss_finish_mn(1, 4, 10, 0, 0, 0, 4, one, 3, None, one, one, None) == nv.ERR_ARG          # combine


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
DEV = "cuda"

# (N, C, K, D, H, W, dtype, Cs): odd and non-cubic extents, fp16 / fp32, padded rows, K <= C <= 64
SHAPES = [
    (1, 2, 2, 7, 5, 9, torch.float16, 2),
    (2, 16, 16, 12, 16, 20, torch.float16, 16),
    (3, 5, 4, 9, 11, 6, torch.float32, 5),
    (2, 13, 13, 17, 6, 10, torch.float16, 16),
    (2, 24, 20, 8, 13, 7, torch.float32, 24),
    (1, 64, 64, 33, 9, 5, torch.float16, 64),
    (3, 8, 8, 5, 7, 11, torch.float32, 12),
    (2, 40, 31, 70, 3, 4, torch.float16, 48),
]


def _random_case(seed, N, C, D, H, W, multi_hot=False):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.rand(N, C, D, H, W, generator=g) * 16 - 8).half().float()      # |x| <= 8, fp16-representable
    if multi_hot:
        labels = (torch.rand(N, C, D, H, W, generator=g) > 0.8).float()
    else:
        classes = torch.randint(0, C, (N, D, H, W), generator=g)
        classes[torch.rand(N, D, H, W, generator=g) < 0.3] = -1
        labels = labels_from_classes(classes, C)
    return logits, labels


def _channels_last(logits, dtype, Cs):
    N, C, D, H, W = logits.shape
    out = torch.zeros(N, D, H, W, Cs, dtype=dtype)
    out[..., :C] = logits.permute(0, 2, 3, 4, 1).to(dtype)
    return out.to(DEV).contiguous()


def _kernel_value(logits_cl, labels, K):
    from diff_unet_amos_amd import ops
    part = ops.multi_neighbor_partials(logits_cl, labels.to(DEV).contiguous(), K).cpu()
    return float(part[:, :K].sum() / part[:, K].sum()), part


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_kernel_matches_restatement(i):
    N, C, K, D, H, W, dtype, Cs = SHAPES[i]
    logits, labels = _random_case(100 + i, N, C, D, H, W, multi_hot=i % 3 == 2)
    if i == 1:
        labels[1] = 0                                    # a sample without labels: fewer than 2 classes, one entry 0
    if i == 3:                                           # saturation ties: the first of several logits >= 20 wins
        sat = torch.rand(N, C, 1, H, W, generator=torch.Generator().manual_seed(5)) < 0.5
        for d, v in ((2, 20.0), (5, 26.0), (9, 30.0)):
            logits[:, :, d:d + 1] = torch.where(sat, torch.tensor(v), logits[:, :, d:d + 1])
    want = float(multi_neighbor_restated(logits, labels, K))
    got, _ = _kernel_value(_channels_last(logits, dtype, Cs), labels, K)
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)


@pytest.mark.gpu
def test_kernel_matches_the_reference_golden():
    from diff_unet_amos_amd import ops
    for name, logits, labels, K, want in _golden_cases():
        C = logits.shape[1]
        for Cs in (C, C + 8):
            got, _ = _kernel_value(_channels_last(logits, torch.float16, Cs), labels, K)
            assert abs(got - want) <= 1e-5 * abs(want), (name, Cs, got, want)
        if K == C:        # the fused loss with multi_neighbor alone returns the term as it is
            L, _, dcomb = ops.seg_loss_reduce(_channels_last(logits, torch.float16, C), labels.to(DEV), ("multi_neighbor",))
            assert abs(float(L) - want) <= 1e-5 * abs(want) and float(dcomb) == 1.0, (name, float(L), want)


@pytest.mark.gpu
def test_kernel_is_deterministic():
    logits, labels = _random_case(7, 2, 16, 20, 24, 28)
    x = _channels_last(logits, torch.float16, 16)
    _, a = _kernel_value(x, labels, 16)
    _, b = _kernel_value(x, labels, 16)
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("combine", ["sum", "mean", "log"])
def test_fused_loss_with_the_amos_set(combine):
    """Value and gradient (times 3) of _SegLoss over the four names against oracle autograd plus the restated term: the
    gradient is that of mse + bce + dice scaled by the combine's derivative over FOUR terms (1/4 under "mean",
    1/(1 + total) with the multi_neighbor term inside the total under "log")."""
    from diff_unet_amos_amd.training import _SegLoss
    g = torch.Generator().manual_seed(23)
    C = 6
    logits_ncdhw = (torch.rand(2, C, 9, 10, 7, generator=g) * 8 - 4).half().float()
    labels = (torch.rand(2, C, 9, 10, 7, generator=g) > 0.6).float()
    logits = logits_ncdhw.permute(0, 2, 3, 4, 1).contiguous().to(DEV).requires_grad_(True)
    L = _SegLoss.apply(logits, labels.to(DEV), tuple(AMOS.split(",")), combine)
    (L * 3.0).backward()
    p = logits_ncdhw.double().clone().requires_grad_(True)
    want = _amos_criterion(combine)(p, labels.double())
    (want * 3.0).backward()
    L = float(L.detach())
    assert abs(L - float(want)) < 1e-5 * max(1.0, abs(float(want))), (L, float(want))
    wg = p.grad.permute(0, 2, 3, 4, 1)
    assert (logits.grad.cpu().double() - wg).abs().max().item() <= 1e-5 * wg.abs().max().item()
    # against the three-term loss: the same gradient direction, the combine's factor differs
    three = logits.detach().clone().requires_grad_(True)
    (_SegLoss.apply(three, labels.to(DEV), ("mse", "bce", "dice"), "sum") * 3.0).backward()
    assert float(multi_neighbor_restated(logits_ncdhw, labels, C)) > 0.01
    factor = {"sum": 1.0, "mean": 0.25, "log": float(torch.exp(-want))}[combine]      # log: 1 / (1 + total of all four)
    assert torch.allclose(logits.grad.cpu().double(), three.grad.cpu().double() * factor, rtol=1e-4, atol=1e-9)


KW = dict(in_channels=1, out_channels=4, features=(8, 8, 16, 32, 64, 8))


def _train_data(n, seed):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(n, 1, 32, 32, 32, generator=g)
    labels = (torch.rand(n, 4, 32, 32, 32, generator=g) > 0.7).float()
    noise = torch.randn(n, 4, 32, 32, 32, generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    return image, labels, noise, t


def _min_vote_gap(preds):
    """Smallest gap between the largest and second-largest sigmoid of any (n, c, h, w) column: how far the prediction's
    depth votes are from a tie that the GPU / CPU rounding difference of the logits could break either way."""
    s = torch.sigmoid(preds.float()).topk(2, dim=2).values
    return float((s[:, :, 0] - s[:, :, 1]).min())


@pytest.mark.gpu
def test_eager_trainer_step_matches_the_reference_step():
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    from oracle.unet_ref import RefDiffUNet
    dev = torch.device("cuda:0")
    image, labels, noise, t = _train_data(2, 62)      # seed: the widest vote gap of 40..69 (1.9e-5)
    torch.manual_seed(0)
    ref = RefDiffUNet(**KW)
    init = ref.state_dict()
    with torch.no_grad():
        preds = ref(image=image, x=ref.diffusion.q_sample(labels * 2 - 1, t, noise), step=t, pred_type="denoise")
    gap = _min_vote_gap(preds)
    assert gap > 1e-5, f"ill-posed comparison: a prediction column is {gap:.1e} from a depth tie"
    want = float(ref_training_step(ref, image, labels, _amos_criterion("sum"), noise, t))
    net = DiffUNet(**KW)
    net.load_state_dict(init)
    net = net.to(dev)
    tr = NativeConvTrainer(net, lr=0.0, dtype=torch.float32, losses=AMOS, loss_combine="sum")
    got = float(tr.step(image.to(dev), labels.to(dev), noise=noise.to(dev), t=t.to(dev)))
    assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (got, want)
    # and with lr > 0 it learns
    torch.manual_seed(0)
    net2 = DiffUNet(**KW).to(dev)
    tr2 = NativeConvTrainer(net2, lr=1e-3, dtype=torch.float32, losses=AMOS, loss_combine="sum")
    image, labels, noise, t = image.to(dev), labels.to(dev), noise.to(dev), t.to(dev)
    losses = [float(tr2.step(image, labels, noise=noise, t=t)) for _ in range(8)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


@pytest.mark.gpu
def test_graph_trainer_step_equals_the_eager_step():
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    dev = torch.device("cuda:0")
    image, labels, noise, t = (x.to(dev) for x in _train_data(2, 43))
    ts = [t, torch.tensor([700, 20], device=dev), torch.tensor([5, 999], device=dev)]
    runs = []
    for graph in (False, True):
        torch.manual_seed(0)
        net = DiffUNet(**KW).to(dev)
        tr = NativeConvTrainer(net, lr=1e-3, dtype=torch.float32, graph=graph, losses=AMOS, loss_combine="mean")
        runs.append([float(tr.step(image, labels, noise=noise, t=tk)) for tk in ts])
    assert np.allclose(runs[0], runs[1], rtol=1e-6), runs


@pytest.mark.gpu
def test_full_size_step_with_the_amos_set():
    """DiffUNet at 96^3, 16 classes, fp16, batch 2: one trainer step with the AMOS set; the multi_neighbor term the step
    counted equals the restatement on that step's own logits, and the step's loss is the fused three-term loss plus it."""
    from diff_unet_amos_amd import ops
    from diff_unet_amos_amd.diff_unet import DiffUNet
    from diff_unet_amos_amd.training import NativeConvTrainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = DiffUNet(in_channels=1, out_channels=16).to(dev)
    tr = NativeConvTrainer(net, dtype=torch.float16, losses=AMOS, loss_combine="sum")
    seen = []
    tr.module.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().clone()))
    g = torch.Generator(device=dev).manual_seed(3)
    image = torch.rand(2, 1, 96, 96, 96, device=dev, generator=g)
    labels = (torch.rand(2, 16, 96, 96, 96, device=dev, generator=g) > 0.8).float()
    loss = float(tr.step(image, labels))
    assert np.isfinite(loss) and len(seen) == 1
    logits = seen[0]
    three, _, _ = ops.seg_loss_reduce(logits, labels, ("mse", "bce", "dice"), "sum")
    part = ops.multi_neighbor_partials(logits, labels).cpu()
    mn_kernel = float(part[:, :16].sum() / part[:, 16].sum())
    mn_cpu = float(multi_neighbor_restated(logits.permute(0, 4, 1, 2, 3).cpu(), labels.cpu(), 16))
    assert abs(mn_kernel - mn_cpu) <= 1e-5 * abs(mn_cpu), (mn_kernel, mn_cpu)
    assert abs(loss - (float(three) + mn_cpu)) <= 1e-5 * abs(loss), (loss, float(three), mn_cpu)
