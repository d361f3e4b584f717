"""sampler_driver.SamplerDriver without a GPU: a stub plan keeps the real state, seed, table and loop code and replaces what
launches kernels (the hooks, the x_T hand-in and the result conversion) with recorders."""
import pytest
import torch

from diff_unet_amos_amd import _native as nv
from diff_unet_amos_amd.gaussian_diffusion import make_spaced
from diff_unet_amos_amd.sampler_driver import SamplerDriver

T = 5


class _Graph:
    def __init__(self, log):
        self.log = log

    def replay(self):
        self.log.append(("replay",))


class StubPlan(SamplerDriver):
    def __init__(self, finish=0):
        self.N, self.C, self.dims, self.dev = 1, 2, (2, 2, 2), torch.device("cpu")
        self.cx = 4
        self.xin = torch.zeros(1, 2, 2, 2, 8)
        self.temb_table = torch.zeros(1000, 4)
        self.finish, self.log = finish, []
        self._alloc_sampler_state(self.N, self.dims, self.cx, self.dev)

    def refresh_weights(self):
        self.log.append(("refresh_weights",))

    def _reset(self, x_T):
        self.log.append(("reset", x_T))

    def _result(self, want_sum):
        return {"want_sum": want_sum}

    def _one_step(self, mode, row_of_step, coef_table, eps, want_sum):
        self.log.append(("step", mode, row_of_step, coef_table, eps, want_sum))

    def _evaluate(self, rows, out):
        self.log.append(("evaluate", rows))

    def _capture(self, step_fn):
        self.log.append(("capture",))
        return _Graph(self.log)

    def _finish_count(self, kind, T):
        return self.finish

    def _finish(self, first_step, T, run):
        self.log.append(("finish", first_step, T))

    def names(self):
        return [e[0] for e in self.log if e[0] != "refresh_weights"]


@pytest.fixture(scope="module")
def diffusion():
    return make_spaced(1000, [T])


@pytest.fixture
def x_T():
    return torch.zeros(1, 2, 2, 2, 2)


def test_state_buffers():
    p = StubPlan()
    assert p.x_state.shape == p.x_sum.shape == (1, 2, 2, 2, 4) and p.x_state.dtype == p.x_sum.dtype == torch.float32
    assert p.cur_coef.shape == (1, 8) and p.cur_coef.dtype == torch.float32
    assert all(getattr(p, n).shape == (1,) and getattr(p, n).dtype == torch.int32 for n in ("counter", "step_word", "err_word"))
    assert p.seed_word.shape == (1,) and p.seed_word.dtype == torch.int64
    assert p.graphs == {} and p.tables == {}


def test_eager_steps_get_their_noise(diffusion, x_T):
    p = StubPlan()
    draws = [torch.full((1, 2, 2, 2, 2), float(k)) for k in range(T)]
    out = p.sample_loop(diffusion, "ddpm", noise=x_T, step_noise=draws, use_graph=True, seed=1)      # step_noise forces eager mode
    assert p.names() == ["reset"] + ["step"] * T
    steps = [e for e in p.log if e[0] == "step"]
    coef_table, row_of_step = p.tables[(diffusion, "ddpm", 0.0)]
    tmap = diffusion.model_timesteps()
    assert row_of_step.tolist() == [tmap[i] for i in range(T - 1, -1, -1)] and row_of_step.dtype == torch.int32
    assert torch.equal(coef_table, diffusion.ddpm_coef(torch.arange(T - 1, -1, -1)))
    for k, (_, mode, rows, coef, eps, want_sum) in enumerate(steps):
        assert mode == nv.MODE_DDPM and rows is row_of_step and coef is coef_table and want_sum is False
        assert torch.equal(eps, draws[k]) and eps.dtype == torch.float32
    assert out == {"want_sum": False}
    # without step_noise: T eager steps with in-kernel noise; DDIM keeps the sum by default
    p = StubPlan()
    assert p.sample_loop(diffusion, "ddim", noise=x_T, eta=0.3, use_graph=False, seed=1) == {"want_sum": True}
    assert [(e[1], e[4], e[5]) for e in p.log if e[0] == "step"] == [(nv.MODE_DDIM, None, True)] * T
    assert torch.equal(p.tables[(diffusion, "ddim", 0.3)][0], diffusion.ddim_coef(torch.arange(T - 1, -1, -1), 0.3))


def test_snapshots_force_eager_mode(diffusion, x_T, monkeypatch):
    p = StubPlan()
    monkeypatch.setattr("diff_unet_amos_amd.ops.from_channels_last", lambda src, c: ("state after", p.names().count("step"), src, c))
    snaps = {2: None, T: None}
    p.sample_loop(diffusion, "ddpm", noise=x_T, snapshots=snaps, seed=1)
    assert p.names() == ["reset"] + ["step"] * T and not p.graphs
    assert snaps == {2: ("state after", 2, p.x_state, p.C), T: ("state after", T, p.x_state, p.C)}


def test_graph_mode_captures_once_per_key(diffusion, x_T):
    p = StubPlan()
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1)
    assert p.names() == ["reset", "capture", "reset"] + ["replay"] * T        # the state is reset again behind the capture's warm-up
    assert list(p.graphs) == [(diffusion, "ddpm", 0.0, False)]
    del p.log[:]
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=2)                         # same key: nothing captured
    assert p.names() == ["reset"] + ["replay"] * T and len(p.graphs) == 1
    del p.log[:]
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=2, want_sum=True)          # another want_sum: a second graph
    assert p.names() == ["reset", "capture", "reset"] + ["replay"] * T
    assert set(p.graphs) == {(diffusion, "ddpm", 0.0, False), (diffusion, "ddpm", 0.0, True)}
    assert len(p.tables) == 1


def test_finishing_steps(diffusion, x_T):
    p = StubPlan(finish=2)
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1)
    assert p.names() == ["reset", "capture", "reset"] + ["replay"] * (T - 2) + ["finish"]
    assert p.log[-1] == ("finish", T - 2, T)
    p = StubPlan(finish=2)
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1, use_graph=False)
    assert p.names() == ["reset"] + ["step"] * (T - 2) + ["finish"] and p.log[-1] == ("finish", T - 2, T)


def test_first_step_runs_the_tail_of_the_process(diffusion, x_T, monkeypatch):
    """first_step = s: the counter word starts at s (again behind the capture's warm-up), steps s .. T - 1 run, entry j of
    step_noise belongs to step s + j, snapshot keys stay absolute, and the finishing steps keep their place."""
    draws = [torch.full((1, 2, 2, 2, 2), float(k)) for k in range(T - 2)]
    p = StubPlan()
    monkeypatch.setattr("diff_unet_amos_amd.ops.from_channels_last", lambda src, c: ("state after", p.names().count("step")))
    snaps = {3: None, T: None}
    p.sample_loop(diffusion, "ddpm", noise=x_T, step_noise=draws, snapshots=snaps, seed=1, first_step=2)
    assert p.names() == ["reset"] + ["step"] * (T - 2) and int(p.counter.item()) == 2       # the stub's steps do not advance it
    assert [float(e[4].flatten()[0]) for e in p.log if e[0] == "step"] == [0.0, 1.0, 2.0]
    assert snaps == {3: ("state after", 1), T: ("state after", T - 2)}
    with pytest.raises(AssertionError):
        StubPlan().sample_loop(diffusion, "ddpm", noise=x_T, step_noise=draws + draws[:1], seed=1, first_step=2)
    p = StubPlan()
    p.counter.fill_(99)                                                                      # as a warm-up step would leave it
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1, first_step=2)
    assert p.names() == ["reset", "capture", "reset"] + ["replay"] * (T - 2) and int(p.counter.item()) == 2
    p = StubPlan(finish=2)
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1, first_step=1)
    assert p.names() == ["reset", "capture", "reset"] + ["replay"] * (T - 3) + ["finish"] and p.log[-1] == ("finish", T - 2, T)
    p = StubPlan(finish=2)                                                                   # a start inside the finishing steps
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1, first_step=T - 1, use_graph=False)
    assert p.names() == ["reset", "finish"] and p.log[-1] == ("finish", T - 1, T)
    p = StubPlan()                                                                           # the default leaves the word alone
    p.counter.fill_(99)
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1, use_graph=False)
    assert int(p.counter.item()) == 99


def test_first_step_argument_errors(diffusion, x_T):
    for bad in (-1, T, T + 3):
        p = StubPlan()
        with pytest.raises(ValueError, match=rf"first_step={bad}: the process has steps 0 <= k < {T}"):
            p.sample_loop(diffusion, "ddpm", noise=x_T, seed=1, first_step=bad)
        assert p.names() == []
    p = StubPlan()
    with pytest.raises(NotImplementedError, match="fuse_runs"):
        p.sample_loop(diffusion, "ddim", noise=x_T, seed=1, fuse_runs=1, first_step=1)
    assert p.names() == []


def test_seed_draws(diffusion, x_T):
    p = StubPlan()
    torch.manual_seed(123)
    p.sample_loop(diffusion, "ddpm", noise=x_T)                                 # seed=None: one draw from the CPU generator
    after = torch.get_rng_state()
    torch.manual_seed(123)
    want = int(torch.randint(0, 2 ** 62, (1,)).item())
    assert torch.equal(after, torch.get_rng_state())
    assert int(p.seed_word.item()) == want
    p.sample_loop(diffusion, "ddpm", noise=x_T, seed=2 ** 63 + 77)             # a given seed: no draw, masked to 63 bits
    assert torch.equal(after, torch.get_rng_state())
    assert int(p.seed_word.item()) == 77


def test_host_timestep_out_of_range_raises_before_any_hook():
    p = StubPlan()
    x = torch.zeros(1, 2, 2, 2, 2)
    for bad in (1000, -1):
        with pytest.raises(ValueError, match=r"timestep out of range: the model was built for 0 <= t < 1000, got \[-?\d+\]"):
            p.denoise(x, torch.tensor([bad]))
    assert p.names() == [] and not p.xin.any()
