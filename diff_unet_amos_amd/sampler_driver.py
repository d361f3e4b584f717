"""What the two launch plans (engine.Plan, swin_engine.SwinPlan) share that is the sampler rather than the network: the
sampler state, the per-call Philox key, the step tables, the reverse loop with its one captured HIP graph per step, the
single denoiser evaluation with its timestep check, and the lazily converted list an encoder pass returns.

A plan supplies ``N, C, cx, dims, dev, xin, temb_table, emb_token, refresh_weights`` and the hooks ``_one_step``, ``_evaluate``
and, where it differs from the default here, ``_capture`` / ``_finish_count`` / ``_finish``."""
from __future__ import annotations

import torch

from . import _native as nv
from . import ops


class LazyEmbeddings(list):
    """What embed_model(image) returns: indexable like the reference's list of 5 NCDHW entries (``_convert(i)`` on first
    access), while the denoiser uses the channels-last device buffers of ``plan``."""

    def __init__(self, plan, token):
        super().__init__([None] * 5)
        self.plan, self.token = plan, token

    def __getitem__(self, i):
        v = super().__getitem__(i)
        if v is None:
            assert self.plan.emb_token == self.token, "embeddings were overwritten by a later encoder pass"
            v = self._convert(i)
            super().__setitem__(i, v)
        return v

    def __iter__(self):
        return (self[i] for i in range(5))


class SamplerDriver:
    def _alloc_sampler_state(self, N, S0, cx, device):
        self.x_state = torch.zeros((N, *S0, cx), dtype=torch.float32, device=device)
        self.x_sum = torch.zeros((N, *S0, cx), dtype=torch.float32, device=device)
        self.cur_coef = torch.zeros((N, 8), dtype=torch.float32, device=device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=device)
        self.step_word = torch.zeros(1, dtype=torch.int32, device=device)
        self.err_word = torch.zeros(1, dtype=torch.int32, device=device)     # set by step_begin on an out-of-range index
        self.seed_word = torch.zeros(1, dtype=torch.int64, device=device)    # Philox key of the current sampling call
        self.graphs = {}
        self.tables = {}

    def new_seed(self, seed=None):
        """Key of this call's in-kernel noise.  The reference draws a fresh th.randn_like every step of every call
        (gaussian_diffusion.py:430,576); the counter-based generator needs a fresh KEY per call for the same effect:
        one draw from torch's CPU generator (so torch.manual_seed governs it), mixed with the rank so that replicas
        do not share a noise field.  The key lives in a device word, not in the captured graph."""
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            try:
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized():
                    seed ^= (dist.get_rank() + 1) * 0x9E3779B97F4A7C15 & (2 ** 62 - 1)
            except Exception:       # pragma: no cover - torch.distributed not built
                pass
        self.seed_word.fill_(int(seed) & (2 ** 63 - 1))
        return seed

    def _step_tables(self, diffusion, kind, eta):
        """(coef_table, row_of_step) of the T reverse steps, on the device."""
        tkey = (diffusion, kind, float(eta))          # the object itself: the table keeps it alive, no id() reuse after GC
        if tkey not in self.tables:
            order = list(range(diffusion.num_timesteps))[::-1]
            tt = torch.tensor(order)
            coef = diffusion.ddpm_coef(tt) if kind == "ddpm" else diffusion.ddim_coef(tt, eta)
            tmap = diffusion.model_timesteps()
            self.tables[tkey] = (coef.to(self.dev).contiguous(),
                                 torch.tensor([tmap[i] for i in order], dtype=torch.int32, device=self.dev))
        return self.tables[tkey]

    def _reset(self, x_T):
        ops.to_channels_last(x_T, self.x_state, 0, self.cx)
        ops.to_channels_last(x_T, self.xin, 0, self.C)
        self.x_sum.zero_()
        self.counter.zero_()

    def _result(self, want_sum):
        return {"sample": ops.from_channels_last(self.x_state, self.C),
                "sum_pred_xstart": ops.from_channels_last(self.x_sum, self.C) if want_sum else None}

    # ---- hooks ------------------------------------------------------------------------------------------
    def _one_step(self, mode, row_of_step, coef_table, eps, want_sum):
        """One reverse step on the current stream: step begin + denoiser + sampler tail (``eps``: this step's draw, None =
        in-kernel noise)."""
        raise NotImplementedError

    def _evaluate(self, rows, out):
        """One denoiser evaluation of the staged ``xin`` at table rows ``rows`` (int32, device) into ``out`` (NCDHW logits)."""
        raise NotImplementedError

    def _capture(self, step_fn):
        """Record ``step_fn`` into a HIP graph; the result has ``replay()``."""
        step_fn()                                   # warm-up outside capture (kernel attributes, caches, workspaces)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step_fn()
        return g

    def _finish_count(self, kind, T):
        """How many of the last steps ``_finish`` runs instead of the loop."""
        return 0

    def _finish(self, first_step, T, run):
        """Steps [first_step, T): ``run(plan, first_step, T)`` steps ``plan`` eagerly."""
        raise NotImplementedError

    # ---- public operations ------------------------------------------------------------------------
    def denoise(self, x, t):
        """logits = model(x, t, image, embeddings) for an already-staged image."""
        self.refresh_weights()
        N = self.N
        assert tuple(x.shape) == (N, self.C, *self.dims) and t.numel() == N
        T = self.temb_table.shape[0]
        on_host = not t.is_cuda
        if on_host and not bool(((t >= 0) & (t < T)).all()):
            raise ValueError(f"timestep out of range: the model was built for 0 <= t < {T}, got {t.tolist()}")
        rows = t.detach().to(device=self.dev, dtype=torch.int32).contiguous()
        if not on_host:
            self.err_word.zero_()
        ops.to_channels_last(x.detach().float().contiguous(), self.xin, 0, self.C)
        out = torch.empty((N, self.C, *self.dims), dtype=torch.float32, device=self.dev)
        self._evaluate(rows, out)
        if not on_host and int(self.err_word.item()):     # device-resident t: the kernel clamped it, say so
            raise ValueError(f"timestep out of range: the model was built for 0 <= t < {T}")
        return out

    def sample_loop(self, diffusion, kind, noise=None, step_noise=None, eta=0.0, use_graph=True, seed=None, want_sum=None,
                    snapshots=None):
        """T reverse steps (T = diffusion.num_timesteps) starting from ``noise`` (x_T, NCDHW) or a fresh draw: the loop bodies
        of p_sample_loop_progressive / ddim_sample_loop_progressive (gaussian_diffusion.py:487-535, 667-716), one captured HIP
        graph replayed per step.  ``step_noise``: optional list of per-step NCDHW draws (parity runs; eager mode); otherwise the
        tail kernel generates eps in-kernel (Philox, keyed per call: ``seed`` or a draw from torch's generator).
        ``snapshots``: optional dict {step count k: None}; after k steps the state x is stored there (NCDHW copy;
        eager mode) -- drift-versus-step measurements.  ``want_sum``: accumulate the sum of the per-step x0 predictions (what
        models/diffusion/diffusion.py:94-98 sums from ``all_samples``); default: DDIM loops only -- the reference's p_sample_loop
        (gaussian_diffusion.py:441-485) returns the final sample alone, and the sum is 113 MB of HBM traffic per step at 96^3 x 16.
        Returns dict(sample, sum_pred_xstart (None without the sum))."""
        want_sum = (kind == "ddim") if want_sum is None else bool(want_sum)
        self.refresh_weights()
        T = diffusion.num_timesteps
        shape = (self.N, self.C, *self.dims)
        if noise is None:
            noise = torch.randn(*shape, device=self.dev)
        assert tuple(noise.shape) == shape
        x_T = noise.detach().float().contiguous()
        self._reset(x_T)
        mode = nv.MODE_DDPM if kind == "ddpm" else nv.MODE_DDIM
        coef_table, row_of_step = self._step_tables(diffusion, kind, eta)
        self.new_seed(seed)
        if step_noise is not None:
            assert len(step_noise) == T
        if step_noise is not None or snapshots:
            use_graph = False

        def run(plan, first, last):
            for k in range(first, last):
                eps = None if step_noise is None else step_noise[k].detach().to(self.dev).float().contiguous()
                plan._one_step(mode, row_of_step, coef_table, eps, want_sum)
                if snapshots and (k + 1) in snapshots:
                    snapshots[k + 1] = ops.from_channels_last(plan.x_state, self.C)

        finish = self._finish_count(kind, T)
        if not use_graph:
            run(self, 0, T - finish)
        else:
            gkey = (diffusion, kind, float(eta), want_sum)
            g = self.graphs.get(gkey)
            if g is None:
                g = self.graphs[gkey] = self._capture(lambda: self._one_step(mode, row_of_step, coef_table, None, want_sum))
                self._reset(x_T)                    # the warm-up step advanced the state
            for _ in range(T - finish):
                g.replay()
        if finish:
            self._finish(T - finish, T, run)
        return self._result(want_sum)
