"""What the two launch plans (engine.Plan, swin_engine.SwinPlan) share that is the sampler rather than the network: the
sampler state, the per-call Philox key, the step tables, the reverse loop with its one captured HIP graph per step, the
single denoiser evaluation with its timestep check, and the lazily converted list an encoder pass returns.

A plan supplies ``N, C, cx, dims, dev, xin, temb_table, emb_token, refresh_weights`` and the hooks ``_one_step``, ``_evaluate``
and, where it differs from the default here, ``_capture`` / ``_finish_count`` / ``_finish``; ``_one_step_logits`` is the step of a
loop that fuses repeated runs (``sample_loop(fuse_runs=R)``: Step-Uncertainty Fusion, include/dua_hip.h)."""
from __future__ import annotations

import torch

from . import _native as nv
from . import ops
from .gaussian_diffusion import suf_step_coef


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

    def _one_step_logits(self, mode, row_of_step, coef_table, eps, logits):
        """``_one_step`` without the running sum that also writes the step's raw model output into ``logits`` (fp32 NCDHW): the
        step of a loop with ``fuse_runs``.  Called only then, so a loop without fusion sees exactly the hooks it always did."""
        raise NotImplementedError

    def _accumulate_runs(self, logits, acc, step_coef):
        """Fold the step that just ran into ``acc``: dua_suf_accumulate at the step index step begin left in ``step_word``."""
        ops.suf_accumulate(logits, acc, step_coef, step_word=self.step_word, err_word=self.err_word)

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

    def _fusion_state(self, diffusion, R):
        """(logits, acc, step_coef) of a loop that fuses R runs: persistent, allocated before any capture.  logits [N, C, ...] is
        what every step's tail writes, acc [N / R, C, ...] the fused result, step_coef the table a_k of this process."""
        shape = (self.N, self.C, *self.dims)
        if getattr(self, "suf_logits", None) is None:
            own = getattr(self, "logits", None)          # a plan that already keeps an NCDHW logits buffer lends it
            ok = own is not None and tuple(own.shape) == shape and own.dtype == torch.float32
            self.suf_logits = own if ok else torch.zeros(shape, dtype=torch.float32, device=self.dev)
            self.suf_acc = {}
        if R not in self.suf_acc:
            self.suf_acc[R] = torch.zeros((self.N // R, *shape[1:]), dtype=torch.float32, device=self.dev)
        tkey = (diffusion, "suf")
        if tkey not in self.tables:
            self.tables[tkey] = suf_step_coef(diffusion.num_timesteps, self.dev)
        return self.suf_logits, self.suf_acc[R], self.tables[tkey]

    def sample_loop(self, diffusion, kind, noise=None, step_noise=None, eta=0.0, use_graph=True, seed=None, want_sum=None,
                    snapshots=None, fuse_runs=None, step_logits=None, first_step=0):
        """T reverse steps (T = diffusion.num_timesteps) starting from ``noise`` (x_T, NCDHW) or a fresh draw: the loop bodies
        of p_sample_loop_progressive / ddim_sample_loop_progressive (gaussian_diffusion.py:487-535, 667-716), one captured HIP
        graph replayed per step.  ``step_noise``: optional list of per-step NCDHW draws (parity runs; eager mode); otherwise the
        tail kernel generates eps in-kernel (Philox, keyed per call: ``seed`` or a draw from torch's generator).
        ``snapshots``: optional dict {step count k: None}; after k steps the state x is stored there (NCDHW copy;
        eager mode) -- drift-versus-step measurements.  ``want_sum``: accumulate the sum of the per-step x0 predictions (what
        models/diffusion/diffusion.py:94-98 sums from ``all_samples``); default: DDIM loops only -- the reference's p_sample_loop
        (gaussian_diffusion.py:441-485) returns the final sample alone, and the sum is 113 MB of HBM traffic per step at 96^3 x 16.
        ``fuse_runs`` = R (DDIM only): the batch is N / R windows of R runs each, rows g R .. g R + R - 1 belonging to window g
        (every row with its own x_T), and each step is followed by the Step-Uncertainty Fusion of its R model outputs
        (dua_suf_accumulate, include/dua_hip.h has the formula) in the same captured graph; no plain sum is kept, and the
        result carries ``fused_pred_xstart`` (NCDHW [N / R, C, ...]).  R = 1 is not the plain sum: the steps are still weighted.
        ``step_logits``: optional list; with ``fuse_runs`` (eager mode) a copy of every step's logits is appended to it.
        ``first_step`` = s: ``noise`` is the state after s steps and the loop runs steps s .. T - 1 only (the tail of a long
        process); ``step_noise`` then has T - s entries, entry j belonging to step s + j, and ``snapshots`` keys stay absolute
        step counts.  The in-kernel noise is keyed by (seed, step), so resuming from a snapshot repeats the full run's bits.
        Returns dict(sample, sum_pred_xstart (None without the sum))."""
        fuse = None
        first_step = int(first_step)
        if not 0 <= first_step < diffusion.num_timesteps:
            raise ValueError(f"first_step={first_step}: the process has steps 0 <= k < {diffusion.num_timesteps}")
        if fuse_runs is not None:
            if first_step:
                raise NotImplementedError("fuse_runs: the fused sum runs over all steps, first_step must be 0")
            R = int(fuse_runs)
            if kind != "ddim":
                raise NotImplementedError("fuse_runs: Step-Uncertainty Fusion is defined for the DDIM loop only")
            if not 1 <= R <= nv.SUF_MAX_RUNS or self.N % R:
                raise ValueError(f"fuse_runs={fuse_runs}: the plan's batch of {self.N} is not a whole number of windows of "
                                 f"1 <= R <= {nv.SUF_MAX_RUNS} runs")
            if self._finish_count(kind, diffusion.num_timesteps):
                raise NotImplementedError("fuse_runs: finishing steps on a companion plan are not fused")
            want_sum = False
        want_sum = (kind == "ddim") if want_sum is None else bool(want_sum)
        self.refresh_weights()
        if fuse_runs is not None:
            fuse = self._fusion_state(diffusion, R)
        T = diffusion.num_timesteps
        shape = (self.N, self.C, *self.dims)
        if noise is None:
            noise = torch.randn(*shape, device=self.dev)
        assert tuple(noise.shape) == shape
        x_T = noise.detach().float().contiguous()
        self._reset(x_T)
        if first_step:
            self.counter.fill_(first_step)
        mode = nv.MODE_DDPM if kind == "ddpm" else nv.MODE_DDIM
        coef_table, row_of_step = self._step_tables(diffusion, kind, eta)
        self.new_seed(seed)
        if step_noise is not None:
            assert len(step_noise) == T - first_step
        if step_noise is not None or snapshots or step_logits is not None:
            use_graph = False
        if fuse is not None:
            return self._fused_loop(fuse, R, diffusion, mode, coef_table, row_of_step, x_T, step_noise, eta, use_graph, snapshots,
                                    step_logits)

        def run(plan, first, last):
            for k in range(first, last):
                eps = None if step_noise is None else step_noise[k - first_step].detach().to(self.dev).float().contiguous()
                plan._one_step(mode, row_of_step, coef_table, eps, want_sum)
                if snapshots and (k + 1) in snapshots:
                    snapshots[k + 1] = ops.from_channels_last(plan.x_state, self.C)

        finish = min(self._finish_count(kind, T), T - first_step)
        if not use_graph:
            run(self, first_step, T - finish)
        else:
            gkey = (diffusion, kind, float(eta), want_sum)
            g = self.graphs.get(gkey)
            if g is None:
                g = self.graphs[gkey] = self._capture(lambda: self._one_step(mode, row_of_step, coef_table, None, want_sum))
                self._reset(x_T)                    # the warm-up step advanced the state
                if first_step:
                    self.counter.fill_(first_step)
            for _ in range(T - finish - first_step):
                g.replay()
        if finish:
            self._finish(T - finish, T, run)
        return self._result(want_sum)

    def _fused_loop(self, fuse, R, diffusion, mode, coef_table, row_of_step, x_T, step_noise, eta, use_graph, snapshots, step_logits):
        """The loop of ``sample_loop(fuse_runs=R)``: T times (step with logits, accumulate), eagerly or from one captured graph."""
        logits, acc, step_coef = fuse
        T = diffusion.num_timesteps

        def step(eps=None):
            self._one_step_logits(mode, row_of_step, coef_table, eps, logits)
            self._accumulate_runs(logits, acc, step_coef)

        acc.zero_()
        if not use_graph:
            for k in range(T):
                step(None if step_noise is None else step_noise[k].detach().to(self.dev).float().contiguous())
                if step_logits is not None:
                    step_logits.append(logits.clone())
                if snapshots and (k + 1) in snapshots:
                    snapshots[k + 1] = ops.from_channels_last(self.x_state, self.C)
        else:
            gkey = (diffusion, "ddim", float(eta), False, "fuse_runs", R)
            g = self.graphs.get(gkey)
            if g is None:
                g = self.graphs[gkey] = self._capture(step)
                self._reset(x_T)                    # the warm-up step advanced the state and the fused sum
                acc.zero_()
            for _ in range(T):
                g.replay()
        out = self._result(False)
        out["fused_pred_xstart"] = acc.clone()
        return out
