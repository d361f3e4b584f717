"""Gradient-norm clipping and the EMA of the weights in NativeConvTrainer (training.py): the captured step against the eager one,
the library's launches against the torch-operator form (clip_grad_norm_ + torch.optim.AdamW + update_ema), overflow steps, the
EMA around the capture's warm-up, evaluation under the EMA weights, files, the untouched default path, and two ranks.  The net and
the 32^3 batches are those of tests/test_training_harness.py."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from diff_unet_amos_amd.diff_unet import DiffUNet

gpu = pytest.mark.gpu
KW = dict(in_channels=1, out_channels=2, features=(8, 8, 16, 32, 64, 8))
RATE = 0.99
NEW_ENTRIES = ("dua_adamw_step_ex", "dua_grads_sumsq", "dua_grad_norm_finish")


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(n, 1, 32, 32, 32, generator=g)
    labels = (torch.rand(n, 2, 32, 32, 32, generator=g) > 0.7).float()
    noise = torch.randn(n, 2, 32, 32, 32, generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    return image, labels, noise, t


def _trainer(dev="cuda:0", **kw):
    from diff_unet_amos_amd.training import NativeConvTrainer
    torch.manual_seed(0)
    net = DiffUNet(**KW).to(dev)
    return net, NativeConvTrainer(net, lr=1e-3, **kw)


def _batch(seed, dev="cuda:0"):
    return tuple(x.to(dev) for x in _data(2, seed))


def _rel(a, b, init):
    """|| (a - init) - (b - init) || / || a - init || over all tensors: how different two walks from ``init`` are."""
    num = sum(float(((x - y).double() ** 2).sum()) for x, y in zip(a, b))
    den = sum(float(((x - z).double() ** 2).sum()) for x, z in zip(a, init))
    return (num / den) ** 0.5


@pytest.fixture(scope="module")
def walks():
    """Four steps on the same batches, timesteps and noise in every form, run once: the torch-operator path with the options
    off / on, the library path eager off / on, the captured step with the options on.  ``max_grad_norm`` is half the first-step
    norm the torch-operator path reports."""
    dev = torch.device("cuda:0")
    image, labels, noise, _ = _batch(31)
    ts = [torch.tensor([100 + 37 * k, 900 - 53 * k], device=dev) for k in range(4)]
    net, tr = _trainer(dtype=torch.float32, fused_optimizer=False, max_grad_norm=float("inf"))
    init = [p.detach().clone() for p in tr.params]
    tr.step(image, labels, noise=noise, t=ts[0])
    first_norm = tr.grad_norm()
    assert math.isfinite(first_norm) and first_norm > 0 and tr.clip_coef() == 1.0
    max_norm = 0.5 * first_norm
    out = dict(init=init, max_norm=max_norm)
    forms = dict(torch_off=dict(fused_optimizer=False), lib_off=dict(),
                 torch_on=dict(fused_optimizer=False, max_grad_norm=max_norm, ema_rate=RATE),
                 lib_on=dict(max_grad_norm=max_norm, ema_rate=RATE), graph_on=dict(graph=True, max_grad_norm=max_norm, ema_rate=RATE))
    for name, kw in forms.items():
        net, tr = _trainer(dtype=torch.float32, **kw)
        losses, norms, coefs = [], [], []
        for tk in ts:
            losses.append(float(tr.step(image, labels, noise=noise, t=tk)))
            if tr.max_grad_norm is not None:
                norms.append(tr.grad_norm()); coefs.append(tr.clip_coef())
        out[name] = dict(losses=losses, norms=norms, coefs=coefs, params=[p.detach().clone() for p in tr.params],
                         ema=None if tr.ema is None else [e.clone() for e in tr.ema])
    return out


@gpu
def test_captured_step_with_clip_and_ema_walks_with_the_eager_one(walks):
    """Whole steps, eager against captured: the losses and grad_norm() to rtol 1e-6, clipping engaged in both.  The parameters
    and the EMA of two whole-step walks are NOT compared at 1e-6 here: the backward kernels add weight gradients with float
    atomics, a last-bit difference in a gradient whose true value is zero (the bias of a convolution that InstanceNorm follows)
    flips the sign of Adam's step for that element, and the relative four-step difference of two runs of the SAME code then
    takes one of a few discrete values -- over 20 processes: 0 (9 times), 8e-8 .. 9e-8 (3), 2.0e-6 (1), 7.2e-4 (7); the EMA
    0, 2.4e-7 .. 2.7e-7, 4.7e-6, 2.6e-4; with or without the weight-gradient side stream -- while the losses were equal to the
    bit and the norms within 1.0e-7 every time.  What the update itself does, eager against captured, is compared bit for bit
    on fixed gradients in test_captured_update_equals_the_eager_one_bit_for_bit; the gaps are printed here."""
    e, g, init = walks["lib_on"], walks["graph_on"], walks["init"]
    p_gap, e_gap = _rel(e["params"], g["params"], init), _rel(e["ema"], g["ema"], init)
    print(f"eager vs graph, clip + EMA: parameters {p_gap:.3e}, EMA {e_gap:.3e}; norms {e['norms']} coefs {e['coefs']}")
    assert np.allclose(e["losses"], g["losses"], rtol=1e-6), (e["losses"], g["losses"])
    assert np.allclose(e["norms"], g["norms"], rtol=1e-6), (e["norms"], g["norms"])
    assert min(e["coefs"]) < 1.0 and min(g["coefs"]) < 1.0          # clipping was engaged
    assert abs(e["norms"][0] - 2 * walks["max_norm"]) <= 1e-4 * e["norms"][0]


@gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["fp32", "loss-scaled"])
def test_captured_update_equals_the_eager_one_bit_for_bit(scaled):
    """The update of a step -- ops.grad_norm, NativeAdamW.step with clip and EMA, adamw_advance: NativeConvTrainer._native_update,
    what every native mode runs after the all-reduce -- issued eagerly and replayed from a HIP graph, four times on the same
    four sets of fixed gradients: parameters, EMA, norm and coefficient are equal to the bit after every update (nothing after
    the all-reduce uses an atomic).  The loss-scaled form passes the scale and the growth counter, as fp16 and captured steps do."""
    gen = torch.Generator().manual_seed(17)
    runs = []
    for captured in (False, True):                     # eager first: every kernel is loaded before the capture
        net, tr = _trainer(dtype=torch.float32, max_grad_norm=1.0, ema_rate=RATE)
        tr.optimizer.materialize_state()
        if not runs:
            fixed = [[(torch.randn(p.shape, generator=gen) * (1024.0 if scaled else 1.0)).to(p.device) for p in tr.params]
                     for _ in range(4)]
        for p in tr.params:
            p.grad = torch.zeros_like(p)
        st = tr._amp_state()
        dev = tr.params[0].device
        scale = torch.full((), 1024.0, device=dev) if scaled else None
        growth = torch.zeros((), dtype=torch.int32, device=dev) if scaled else None
        update = lambda: tr._native_update(scale, st["flag"], growth, st["seen"])      # noqa: E731
        graph = None
        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                update()
        trace = []
        for grads in fixed:
            for p, g in zip(tr.params, grads):
                p.grad.copy_(g)
            graph.replay() if captured else update()
            assert not tr.last_step_overflowed() and 0.0 < tr.clip_coef() < 1.0
            trace.append(([p.detach().clone() for p in tr.params], [e.clone() for e in tr.ema], tr.grad_norm(), tr.clip_coef()))
        assert int(tr.optimizer._count) == 4
        runs.append(trace)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a[2] == b[2] and a[3] == b[3], (k, a[2:], b[2:])
        assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])), k
    assert any(not torch.equal(x, y) for x, y in zip(runs[0][0][0], runs[0][3][0]))          # and the walk moved


@gpu
@pytest.mark.parametrize("mode", ["eager-fp32", "eager-fp16", "graph"])
def test_ema_alone_without_clipping(mode):
    """``ema_rate`` with ``max_grad_norm=None`` (the reference's own configuration): the overflow check stays grads_nonfinite,
    the step is the EMA-only form of the kernel, and after each step e' = fl(e + fl(w fl(p' - e))) on the step's own p'."""
    net, tr = _trainer(dtype=torch.float16 if mode == "eager-fp16" else torch.float32, graph=mode == "graph", ema_rate=RATE)
    image, labels, noise, t = _batch(5)
    assert tr._gn is None
    with pytest.raises(RuntimeError):
        tr.grad_norm()
    w = torch.tensor(1.0 - RATE, dtype=torch.float64).float().to("cuda:0")
    for _ in range(2):
        before = [e.clone() for e in tr.ema]
        tr.step(image, labels, noise=noise, t=t)
        assert not tr.last_step_overflowed()
        for e, p, q in zip(tr.ema, tr.params, before):
            assert torch.equal(e, q + w * (p.detach() - q))
    assert any(not torch.equal(e, p.detach()) for e, p in zip(tr.ema, tr.params))


@gpu
def test_library_clip_and_ema_walk_like_the_torch_operators(walks):
    """The parent's gap between torch.optim.AdamW and the library's AdamW (options off) against the gaps with the options on:
    clipping rescales a gradient that Adam normalises away again and the EMA is a linear filter of the parameter walk, so
    neither may widen it by more than the factor two allowed for the different first-step sign pattern."""
    init = walks["init"]
    base = _rel(walks["torch_off"]["params"], walks["lib_off"]["params"], init)
    p_gap = _rel(walks["torch_on"]["params"], walks["lib_on"]["params"], init)
    e_gap = _rel(walks["torch_on"]["ema"], walks["lib_on"]["ema"], init)
    print(f"torch operators vs library, four steps: options off {base:.3e}; clip + EMA on: parameters {p_gap:.3e}, EMA {e_gap:.3e}")
    assert min(walks["torch_on"]["coefs"]) < 1.0 and min(walks["lib_on"]["coefs"]) < 1.0
    assert np.allclose(walks["torch_on"]["norms"][0], walks["lib_on"]["norms"][0], rtol=1e-5)
    assert p_gap <= 2 * base and e_gap <= 2 * base, (base, p_gap, e_gap)


@gpu
def test_grad_norm_reads_back_the_norm_of_the_stored_gradient():
    net, tr = _trainer(dtype=torch.float16, max_grad_norm=float("inf"))
    image, labels, noise, t = _batch(11)
    tr.step(image, labels, noise=noise, t=t)                       # the eager fp16 step stores the unscaled gradient
    assert not tr.last_step_overflowed() and tr.clip_coef() == 1.0
    want = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in tr.params))
    assert want > 0 and abs(tr.grad_norm() - want) <= 1e-6 * want, (tr.grad_norm(), want)


@gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_overflow_step_leaves_parameters_and_ema_alone(graph):
    net, tr = _trainer(dtype=torch.float16, graph=graph, init_scale=2.0 ** 40, max_grad_norm=1.0, ema_rate=RATE)
    image, labels, noise, t = _batch(11)
    with torch.no_grad():
        for e in tr.ema:                                           # an EMA that differs from the weights: a skipped lerp shows
            e.mul_(0.5)
    p0, e0 = [p.detach().clone() for p in tr.params], [e.clone() for e in tr.ema]
    tr.step(image, labels, noise=noise, t=t)
    assert tr.last_step_overflowed() and tr.loss_scale() == 2.0 ** 39
    assert not math.isfinite(tr.grad_norm()) and tr.clip_coef() == 0.0
    assert all(torch.equal(a, b) for a, b in zip(tr.params, p0)) and all(torch.equal(a, b) for a, b in zip(tr.ema, e0))
    for _ in range(40):
        tr.step(image, labels, noise=noise, t=t)
        if not tr.last_step_overflowed():
            break
    assert not tr.last_step_overflowed() and math.isfinite(tr.grad_norm())
    moved_p = sum(int(not torch.equal(a, b)) for a, b in zip(tr.params, p0))
    moved_e = sum(int(not torch.equal(a, b)) for a, b in zip(tr.ema, e0))
    assert moved_p > 0.9 * len(p0) and moved_e > 0.9 * len(e0), (moved_p, moved_e)


@gpu
def test_ema_survives_the_capture_and_a_load_keeps_its_addresses():
    """After the first captured step the EMA is ONE update of a copy of the initial weights (the three warm-up updates left no
    trace); load_ema_state_dict copies into the live tensors, and the next replay updates what was loaded."""
    net, tr = _trainer(dtype=torch.float32, graph=True, max_grad_norm=1.0, ema_rate=RATE)
    image, labels, noise, t = _batch(5)
    init = [p.detach().clone() for p in tr.params]
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(tr.ema, tr.params))
    tr.step(image, labels, noise=noise, t=t)
    w = torch.tensor(1.0 - RATE, dtype=torch.float64).float().to("cuda:0")            # (float)(1.0 - rate)
    for e, p, q in zip(tr.ema, tr.params, init):
        assert torch.equal(e, q + w * (p.detach() - q))                                 # fl(e + fl(w fl(p' - e))), e = the initial weight
    ptrs = [e.data_ptr() for e in tr.ema]
    sd = {k: torch.full_like(v, 0.25) for k, v in tr.ema_state_dict().items()}
    tr.load_ema_state_dict(sd)
    assert [e.data_ptr() for e in tr.ema] == ptrs and all(bool((e == 0.25).all()) for e in tr.ema)
    tr.step(image, labels, noise=noise, t=t)
    for e, p in zip(tr.ema, tr.params):
        assert torch.equal(e, 0.25 + w * (p.detach() - 0.25))


@gpu
def test_evaluation_under_the_ema_weights(tmp_path):
    """Inside ``ema_weights()`` the engine's forward is, bit for bit, that of a second net loaded from ema_state_dict(); after the
    block the parameters, the EMA, the moments and the update counter are back to the bit at their addresses -- the next training
    step is the uninterrupted run's step on the uninterrupted run's state -- and that step still updates the live EMA.  save_ema /
    load_ema round-trip the state dict under the reference's file name."""
    from diff_unet_amos_amd import checkpoint
    image, labels, noise, t = _batch(5)
    runs = []
    for interrupt in (False, True):
        net, tr = _trainer(dtype=torch.float32, graph=True, max_grad_norm=1.0, ema_rate=RATE)
        init = [p.detach().clone() for p in tr.params]
        for _ in range(2):
            tr.step(image, labels, noise=noise, t=t)
        if interrupt:
            before = [p.detach().clone() for p in tr.params]
            live_state = [st[k] for q in tr.params for st in [tr.optimizer.state[q]] for k in ("exp_avg", "exp_avg_sq")]
            moments = [x.clone() for x in live_state]
            ptrs = [t_.data_ptr() for t_ in (*tr.params, *tr.ema, *live_state)]
            sd = tr.ema_state_dict()
            assert list(sd) == list(net.state_dict())
            path = checkpoint.save_ema(str(tmp_path), sd, RATE, 2)
            assert os.path.basename(path) == "ema_0.99_000002.pt" == checkpoint.ema_filename(RATE, 2)
            loaded = checkpoint.load_ema(path, map_location="cuda:0")
            assert list(loaded) == list(sd) and all(torch.equal(loaded[k], sd[k]) for k in sd)
            torch.manual_seed(0)
            other = DiffUNet(**KW).to("cuda:0")
            other.load_state_dict(loaded)
            with torch.no_grad():
                torch.manual_seed(3)
                want = other(image, pred_type="ddim_sample")
                with tr.ema_weights():
                    assert all(torch.equal(p.detach(), loaded[k]) for k, p in zip(tr._param_names, tr.params))
                    torch.manual_seed(3)
                    got = net(image, pred_type="ddim_sample")
                torch.manual_seed(3)
                live = net(image, pred_type="ddim_sample")
            assert torch.equal(got, want) and not torch.equal(live, want)
            assert all(torch.equal(p.detach(), b) for p, b in zip(tr.params, before))
            assert all(torch.equal(e, loaded[k]) for k, e in zip(tr._param_names, tr.ema))
            # ... and so is everything else the next step reads, at the addresses the captured step was given
            state = [st[k] for q in tr.params for st in [tr.optimizer.state[q]] for k in ("exp_avg", "exp_avg_sq")]
            assert all(torch.equal(a, b) for a, b in zip(state, moments)) and int(tr.optimizer._count) == 2
            assert [t_.data_ptr() for t_ in (*tr.params, *tr.ema, *state)] == ptrs
        e_before = [e.clone() for e in tr.ema]
        loss = float(tr.step(image, labels, noise=noise, t=t))
        w = torch.tensor(1.0 - RATE, dtype=torch.float64).float().to("cuda:0")
        for e, q, b in zip(tr.ema, tr.params, e_before):                    # the replay still updates the live tensors
            assert torch.equal(e, b + w * (q.detach() - b))
        runs.append((loss, [q.detach().clone() for q in tr.params], [e.clone() for e in tr.ema]))
    # The block left every tensor the step reads as it was, to the bit and at its address: the next step is the uninterrupted
    # run's step on the uninterrupted run's state.  Two runs of it are still two backward passes with float atomics (see
    # test_captured_step_with_clip_and_ema_walks_with_the_eager_one), so across the runs only the loss is asserted; the gaps are printed.
    p_gap, e_gap = _rel(runs[0][1], runs[1][1], init), _rel(runs[0][2], runs[1][2], init)
    print(f"uninterrupted vs interrupted by an evaluation under the EMA weights, three steps: parameters {p_gap:.3e}, EMA {e_gap:.3e}")
    assert np.allclose(runs[0][0], runs[1][0], rtol=1e-6), (runs[0][0], runs[1][0])


class _Counting:
    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1
        return getattr(self._real, name)


@gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_defaults_issue_none_of_the_new_launches(monkeypatch, graph):
    from diff_unet_amos_amd import _native as nv
    image, labels, noise, t = _batch(5)
    seen = {}
    for on in (False, True):
        proxy = _Counting(nv.lib())
        monkeypatch.setattr(nv, "lib", lambda proxy=proxy: proxy)
        kw = dict(max_grad_norm=1.0, ema_rate=RATE) if on else {}
        net, tr = _trainer(dtype=torch.float16, graph=graph, **kw)
        assert (tr.ema is not None) == on
        for _ in range(2):
            tr.step(image, labels, noise=noise, t=t)
        seen[on] = {k: proxy.calls.get(k, 0) for k in NEW_ENTRIES + ("dua_adamw_step", "dua_grads_nonfinite")}
    print(seen)
    assert all(seen[False][k] == 0 for k in NEW_ENTRIES) and seen[False]["dua_adamw_step"] > 0 and seen[False]["dua_grads_nonfinite"] > 0
    assert all(seen[True][k] > 0 for k in NEW_ENTRIES) and seen[True]["dua_adamw_step"] == 0 and seen[True]["dua_grads_nonfinite"] == 0


def _two_rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)       # both ranks share cuda:0; gloo moves CUDA tensors via the host
    try:
        dev = torch.device("cuda:0")
        net, tr = _trainer(dev, dtype=torch.float32, overlap=False, graph=True, max_grad_norm=1e-3, ema_rate=RATE)
        image, labels, noise, t = _data(2, 8)
        sl = slice(rank, rank + 1)
        norms, coefs = [], []
        for k in range(3):
            tr.step(image[sl].to(dev), labels[sl].to(dev), noise=noise[sl].to(dev), t=((t[sl] + 211 * k) % 1000).to(dev))
            norms.append(tr.grad_norm()); coefs.append(tr.clip_coef())
        q.put((rank, norms, coefs, [p.detach().cpu().numpy() for p in tr.params], [e.cpu().numpy() for e in tr.ema]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@gpu
def test_two_ranks_hold_identical_parameters_ema_and_norm():
    """graph=True (two graphs, the flat all-reduce between them), clipping engaged, EMA on, three steps: the norm is that of the
    averaged gradient and the norm kernels are deterministic, so both ranks derive the same coefficient to the bit."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 733) % 2000
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = {r: rest for r, *rest in (q.get(timeout=300) for _ in range(2))}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (n0, c0, p0, e0), (n1, c1, p1, e1) = outs[0], outs[1]
    print(f"norms {n0} coefs {c0}")
    assert n0 == n1 and c0 == c1 and all(math.isfinite(x) for x in n0) and max(c0) < 1.0
    assert all(np.array_equal(a, b) for a, b in zip(p0, p1)) and all(np.array_equal(a, b) for a, b in zip(e0, e1))
    assert any(not np.array_equal(a, b) for a, b in zip(p0, e0))
