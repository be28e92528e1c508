"""`Trainer` — the reference's stage-2 trainer (trainer/Latent_SDE_Trainer.py), MI355X path.

Kept: `Trainer(cfg, model, compressor, device)`, `score_fn(t, x, label, condition) -> (score, params)` (:57-61),
`val_loss(data, condition) -> held-out denoising loss` (:63-92), `update(data, condition)` / `update_score(eps, condition, cates,
discrete)` — one Score training step: backward, clip, Adam + EMA (:94-141; ldt_amd/train.py) —
`sample(num_samples, num_points, label, condition) -> (points, eps)` (:143-165), `valsample`-style "Sample rate"
timing (:178-181,206), EMA weight swap (:146,164; tools/utils.py:80-101), `save` / `resume` with the reference's checkpoint
dict (:228-266).  Training covers the Score of the shipped YAMLs (LayerNorm, AdaLN, self-attention, unconditional or labelled);
the Compressor and the hybrid objective are not trained on this path.  The steps the methods (and `HybridTrainer`) share are said once:
`_ema_weights`, `_draw_times`, `_diffuse`, `_label`, `_update`; the evaluation loop's pieces are ldt_amd/evalloop.py's.

Multi-GPU: when torch.distributed is initialised, `sample(B)` runs rows [lo,hi) of the batch on this rank and
all-gathers the finished points/latents once (ldt_amd/dist.py); results do not depend on the world size when
every rank seeds the CPU generator identically (the reference's common_init, tools/utils.py:269-276).
"""
import contextlib
import os
import time

import torch

from . import dist as ldist
from . import evalloop
from .diffusion import DiffusionSubVPSDE, DiffusionVESDE, DiffusionVPSDE
from .evalloop import _sync                              # (kept importable from here)


class EMAWeights:
    """The part of tools/utils.py:25-101 (EMA optimizer wrapper) the sampler touches: `state[p]['ema']` and
    `swap_parameters_with_ema`.  With no EMA state (fresh model) the swap is a no-op, as upstream (:93-94)."""

    def __init__(self, params, ema_decay):
        self.ema_decay = ema_decay
        self.apply_ema = ema_decay > 0.
        self.params = list(params)
        self.state = {}

    def load_ema(self, optim_state_dict):
        """Adopt the 'ema' tensors of a reference optimizer state_dict (`score_optim_state_dict`,
        Latent_SDE_Trainer.py:233): its param ids follow parameter order."""
        st = optim_state_dict.get("state", {})
        for i, p in enumerate(self.params):
            if i in st and "ema" in st[i]:
                self.state[p] = {"ema": st[i]["ema"].to(p.device, p.dtype)}

    def swap_parameters_with_ema(self, store_params_in_ema):
        if not self.apply_ema:
            return
        for p in self.params:
            if not p.requires_grad or p not in self.state or "ema" not in self.state[p]:
                continue
            ema = self.state[p]["ema"]
            if store_params_in_ema:
                tmp = p.data.detach()
                p.data = ema.detach()
                self.state[p]["ema"] = tmp
            else:
                p.data = ema.detach()


class Trainer:
    def __init__(self, cfg, model, compressor, device):
        self.cfg = cfg
        if cfg.sde.sde_type == "vpsde":                   # Latent_SDE_Trainer.py:23-28 (any other type leaves no self.SDE upstream)
            self.SDE = DiffusionVPSDE(cfg.sde)
        elif cfg.sde.sde_type == "sub_vpsde":
            self.SDE = DiffusionSubVPSDE(cfg.sde)
        elif cfg.sde.sde_type == "vesde":
            self.SDE = DiffusionVESDE(cfg.sde)
        self.sde_type = cfg.sde.sde_type
        self.num_points = cfg.data.tr_max_sample_points
        self.device = device
        self.num_categorys = cfg.data.num_categorys
        self.model = model.to(device)
        self.compressor = compressor.to(device)
        # Latent_SDE_Trainer.py:42-44: EMA(Adam(...)) and its cosine schedule.  AdamEMA is an EMAWeights; it allocates nothing until the
        # first training step.  (The YAML fields a sampling-only config leaves out take torch.optim.Adam's defaults.)
        from .train import AdamEMA
        opt = cfg.opt
        self.optimizer = AdamEMA(self.model.parameters(), lr=getattr(opt, "lr", 1e-3), betas=(getattr(opt, "beta1", 0.9), getattr(opt, "beta2", 0.999)),
                                 weight_decay=getattr(opt, "weight_decay", 0.), ema_decay=opt.ema_decay)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, getattr(getattr(cfg, "common", None), "epochs", 1), 0)
        self.sample_time_eps = cfg.sde.sample_time_eps
        self.sample_N = cfg.sde.sample_N
        self.sample_mode = cfg.sde.sample_mode
        self.epoch, self.itr, self.time = 1, 0, 0.

    def score_fn(self, t, x, label=None, condition=None):
        t = t.to(x)
        params = self.model(x, t, label=label, condition=condition)
        from . import ops
        sde = self.SDE                                    # score = -params / sqrt(var(t)), one HIP kernel
        if sde.score_kind == 0:
            return ops.vpsde_score(params, t.float(), sde.beta_start, sde.beta_end, sde.sigma2_0), params
        return ops.sde_score(params, t.float(), sde.score_kind, *sde.score_consts()), params

    # ---- what sample, val_loss, update / update_score and HybridTrainer.val_nelbo share -------------------------------
    @contextlib.contextmanager
    def _ema_weights(self, active=True):
        """The EMA weights in for the body and out again, also when the body raises (tools/utils.py:80-101); active=False: nothing."""
        if active:
            self.optimizer.swap_parameters_with_ema(store_params_in_ema=True)
        try:
            yield
        finally:
            if active:
                self.optimizer.swap_parameters_with_ema(store_params_in_ema=True)

    @property
    def timesteps(self):
        """The discrete time grid, host fp32 like the schedule tables."""
        return torch.linspace(1.0, self.sample_time_eps, self.cfg.sde.train_N)

    def _label(self, data):
        return data["cate_idx"].to(self.device) if self.cfg.data.num_categorys > 1 else None

    def _draw_times(self, size, discrete, who, *, t_index=None, iw_mode=None, rho=None):
        """The forward-diffusion times of a batch -> (t, e2int_f, var, iw_weight), host fp32, the first three (size,).
        discrete: ONE `np.random.choice(arange(train_N), size)` on numpy's global generator (none when `t_index` (size,) is given) into
        `timesteps`; iw_weight is None.  Otherwise `SDE.iw_quantities(size, cfg.sde.time_eps, iw_mode, sde_type == 'sub_vpsde')` — one
        `torch.rand(size)` on the CPU generator unless `rho` is given — with its obj_weight_t, shaped as it comes, as iw_weight."""
        if discrete:
            import numpy as np
            if t_index is None:
                t_index = np.random.choice(np.arange(self.cfg.sde.train_N), size, replace=True)
            idx = torch.as_tensor(np.asarray(t_index)).long().reshape(-1)
            if idx.numel() != size:
                raise ValueError("%s: t_index holds %d entries for a batch of %d" % (who, idx.numel(), size))
            t = self.timesteps.index_select(0, idx)
            e2int_f, var, weight = self.SDE.e2int_f(t), self.SDE.var(t), None
        else:
            t, var, e2int_f, weight, _, _ = self.SDE.iw_quantities(size, time_eps=self.cfg.sde.time_eps, iw_sample_mode=iw_mode,
                                                                   iw_subvp_like_vp_sde=self.sde_type == "sub_vpsde", rho=rho)
        return t.reshape(-1).float(), e2int_f.reshape(-1).float(), var.reshape(-1).float(), weight

    def _diffuse(self, eps, t, e2int_f, var, eta, seed):
        """x_t = eps e2int_f(t) + sqrt(var(t)) eta (ldt_diffuse_q) -> (t on the device, xt, eta).  Without `eta` the noise comes from the
        device Philox stream, keyed by `seed` or else by ONE draw of the CPU generator (upstream: `randn_like` on the CUDA generator)."""
        from . import ops
        dev = eps.device
        if eta is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        xt, eta = ops.diffuse_q(eps, e2int_f.to(dev), var.to(dev), None if eta is None else eta.to(dev, torch.float32), seed=seed or 0)
        return t.to(dev), xt, eta

    @torch.no_grad()
    def sample(self, num_samples, num_points=None, label=None, condition=None, *, x0=None, noise=None, seed=None,
               use_graph=None, trajectory=None):
        self.model.eval()
        self.compressor.eval()
        with self._ema_weights():
            if self.sample_mode not in ("discrete", "continuous"):
                raise NotImplementedError("sample_mode %r" % (self.sample_mode,))
            cs = self.cfg.score
            if getattr(cs, "graphconv", False):
                # Latent_SDE_Trainer.py:158 samples (z_scale, z_dim + 3) latents under cfg.score.graphconv, which Score.ln_in —
                # Conv1d(z_dim -> hidden), score.py:110 — then rejects: no shipped YAML sets it; same failure, said plainly
                raise RuntimeError("cfg.score.graphconv=True: the sampler would draw latents with z_dim + 3 = %d channels, but "
                                   "Score.ln_in expects z_dim = %d (the reference fails in conv1d on the same mismatch)"
                                   % (cs.z_dim + 3, cs.z_dim))
            shape = (cs.z_scale, cs.z_dim)
            rank, ws = ldist.world()
            lo, hi, per = ldist.shard_bounds(num_samples, rank, ws)
            # every rank draws the FULL-batch x0 from its (identically seeded) CPU generator, then keeps its rows
            if x0 is None:
                x0 = torch.randn((num_samples,) + shape)
            if seed is None and noise is None and self.sample_mode == "discrete":
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # Philox key (only when device noise will be drawn)
            if ldist.initialized():
                ldist.check_same_draws(x0, seed, self.device)            # world-size invariance needs identical CPU generators
            x0_loc = _rows(x0, lo, hi, per)
            noise_loc = None if noise is None else _rows(noise.transpose(0, 1), lo, hi, per).transpose(0, 1)
            if ws > 1:                                   # per-sample conditioning follows its samples to their rank
                if torch.is_tensor(label):
                    label = _rows(label, lo, hi, per)
                if isinstance(condition, (tuple, list)):
                    condition = tuple(_rows(c, lo, hi, per) if torch.is_tensor(c) else c for c in condition)
                elif isinstance(condition, dict):        # raw ViPC inputs {'img','pts'}: ConditionNet runs on this rank's rows
                    condition = {k: _rows(v, lo, hi, per) if torch.is_tensor(v) else v for k, v in condition.items()}
            if self.sample_mode == "continuous":             # probability-flow ODE (Latent_SDE_Trainer.py:148-152)
                eps, self.nfe_count, _ = self.SDE.sample_model_ode(
                    score_fn=self.score_fn, num_samples=per, shape=(cs.z_scale, cs.z_dim), label=label, ode_eps=self.sample_time_eps,
                    enable_autocast=False, ode_solver_tol=self.cfg.sde.ode_tol, condition=condition, noise=x0_loc, device=self.device,
                    solver=getattr(self.cfg.sde, "ode_solver", None) or os.environ.get("LDT_ODE_SOLVER", "scipy"))
            else:
                eps = self.SDE.sample_discrete(score_fn=self.score_fn, N=self.cfg.sde.sample_N,
                                               corrector=self.cfg.sde.corrector, predictor=self.cfg.sde.predictor,
                                               corrector_steps=self.cfg.sde.corrector_steps, shape=shape,
                                               time_eps=self.sample_time_eps, label=label, denoise=self.cfg.sde.denoise,
                                               device=self.device, num_samples=per,
                                               probability_flow=self.cfg.sde.probability_flow, snr=self.cfg.sde.snr,
                                               condition=condition, x0=x0_loc, noise=noise_loc, sample_offset=lo,
                                               seed=seed, use_graph=use_graph, global_batch=num_samples if ws > 1 else None,
                                               trajectory=trajectory)
            npts = self.num_points if num_points is None else num_points
            sample = self.compressor.sample((per, npts), given_eps=eps)
            if ldist.initialized():                      # the single collective of the path
                sample = ldist.all_gather_rows(sample, num_samples)
                eps = ldist.all_gather_rows(eps, num_samples)
        return sample, eps

    @torch.no_grad()
    def val_loss(self, data, condition=None, *, t_index=None, eta=None, seed=None):
        """The held-out denoising loss of one batch, the reference's method line for line (trainer/Latent_SDE_Trainer.py:63-92;
        train_Latent_Diffusion.py:76 calls it per test batch): inside `_ema_weights`, `compressor(data['te_points'])['all_eps']`, the label
        from `data['cate_idx']` when cfg.data.num_categorys > 1, discrete times (`_draw_times`: so `np.random.seed` reproduces upstream's),
        x_t (`_diffuse`), `params = Score(xt, t, label=, condition=)`, |eta - params| for cfg.opt.loss_type "l1" and the square otherwise,
        the mean over everything (ldt_dsm_loss).  Returns the 0-dim device tensor; nothing is synchronised.  Keyword extensions (not in the
        reference): `t_index` (B,) replaces the numpy draw, `eta` (B, tokens, z) the noise, `seed` the Philox key.  The pieces stay
        available as `self.last_val_loss`."""
        from . import ops
        self.model.eval()
        self.compressor.eval()
        with self._ema_weights():
            eps = self.compressor(data["te_points"].to(self.device))["all_eps"]
            label = self._label(data)
            t, e2int_f, var, _ = self._draw_times(eps.shape[0], True, "val_loss", t_index=t_index)
            t_dev, xt, eta = self._diffuse(eps, t, e2int_f, var, eta, seed)
            params = self.model(xt, t_dev, condition=condition, label=label)
            loss, per_sample = ops.dsm_loss(eta, params, None, l1=self.cfg.opt.loss_type == "l1")
            self.last_val_loss = {"t": t_dev, "eps": eps, "eta": eta, "xt": xt, "params": params, "sample_loss": per_sample}
        return loss

    @torch.no_grad()
    def valsample(self, test_loader, val_cate=0, vis=False, *, batch_size=None, ref=None, save_npy=None):
        """The reference's validation sampling loop, same signature and return value (trainer/Latent_SDE_Trainer.py:167-226;
        called as `trainer.valsample(test_loader=test_loader, val_cate=13)` by train_Latent_Diffusion.py:60,85).

        `test_loader` is any iterable of the dataset's dict batches (`te_points`, `tr_points`, `cate_idx`); the references and the sampled
        batches are `evalloop.collect_refs` / `sample_clouds`: per batch when `cfg.data.num_categorys == 1` (:173-188), otherwise by
        `cate_idx == val_cate` with label-conditioned batches (:189-205; upstream appends `self.sample(...)`'s (points, eps) TUPLE there and
        would fail in `torch.cat`: the points are what is meant), cut to len(ref).  Then the "Sample rate" print (:206) and the
        `smp_ep<epoch>.npy` dump (:207-210), both on rank 0, `compute_all_metrics(smp, ref, batch_size=64)` (:217-220) and its report.  `vis=True` (mitsuba
        rendering, :211-216) is out of scope and raises.

        Keyword extensions (not in the reference): `test_loader` may be an int = that many unconditional batches of
        `batch_size` (default `cfg.data.test_batch_size`) scored against `ref` (N, points, 3) when given; `save_npy`
        False suppresses the dump, None (default) dumps whenever `cfg.log.save_path` is set.  The samples and the rate of
        the last call stay available as `self.last_valsample = {"samples", "refs", "rate"}`."""
        evalloop.refuse_vis("valsample", vis)
        self.model.eval()
        self.compressor.eval()
        dev, d = self.device, self.cfg.data
        if isinstance(test_loader, int):                                   # extension: no dataset at hand
            cate, sizes = None, [batch_size or d.test_batch_size] * test_loader
        else:                                                              # :173-188 per batch, :189-205 by category
            cate = None if d.num_categorys == 1 else val_cate
            ref, sizes, _ = evalloop.collect_refs(test_loader, dev, "valsample", cate, None if cate is None else d.test_batch_size)
        smp, use_time = evalloop.sample_clouds(lambda **kw: self.sample(**kw)[0], sizes, dev, cate)
        if ref is not None:
            ref = ref.to(smp)
            smp = smp[:ref.shape[0]]
        rate = smp.shape[0] / max(use_time, 1e-9)
        chief = ldist.world()[0] == 0
        if chief:
            print("Sample rate: %.8f " % rate)
        self.last_valsample = {"samples": smp, "refs": ref, "rate": rate}
        if save_npy and not (getattr(self.cfg.log, "save_path", "") or ""):
            raise ValueError("valsample(save_npy=True) needs cfg.log.save_path (upstream writes smp_ep<epoch>.npy there)")
        if save_npy is not False:
            evalloop.dump(self.cfg, "smp_ep%d" % self.epoch + ".npy", smp, chief)
        if ref is None:
            return {}
        from .metrics import compute_all_metrics
        return evalloop.report(self.epoch, compute_all_metrics(smp, ref, batch_size=64), chief)

    # ---- training: one Score step (trainer/Latent_SDE_Trainer.py:94-141, trainer/base.py:32-37) -------------------
    def warm_up(self, optimizer, itr):
        evalloop.warm_up(self.cfg, optimizer, itr)

    def update(self, data, condition=None):
        """The reference's `update` line for line (:94-109): labels from `data['cate_idx']` when cfg.data.num_categorys > 1, then
        `_update` on `data['tr_points']` with cfg.opt.discrete (default False).  Returns the 0-dim device loss."""
        from .train import refuse_untrainable
        refuse_untrainable(self.model, condition, ldist.world()[1])
        self._refuse_host("Trainer.update")
        return self._update(self._label(data), data["tr_points"], getattr(self.cfg.opt, "discrete", False), condition)

    def _refuse_host(self, who):
        if not torch.device(self.device).type == "cuda" or not torch.cuda.is_available():
            raise RuntimeError("%s: device %s; the HIP path has no CPU fallback" % (who, self.device))

    def _update(self, cates, point, discrete, condition):
        """What `update` is after its refusals: the EMA swap around the step from the second iteration on, the frozen Compressor's
        `all_eps` of the points, `update_score`, `itr += 1` (a raise leaves `itr` as it was)."""
        with self._ema_weights(self.itr > 0):
            with torch.no_grad():
                self.compressor.eval()
                eps = self.compressor(point.to(self.device))["all_eps"]
            loss = self.update_score(eps, cates=cates, discrete=discrete, condition=condition)
        self.itr += 1
        return loss

    def update_score(self, eps, condition=None, cates=None, discrete=False, *, t_index=None, eta=None, seed=None):
        """The reference's `update_score` (:111-141): warm-up of the learning rate, the times (`_draw_times`: the discrete grid, or
        cfg.sde.iw_sample_p_mode with its per-sample `weight_p`), x_t (`_diffuse`), the Score in training mode with its activations kept, the
        l1 / l2 loss (ldt_dsm_loss), the backward pass, `clip_grad_norm_(cfg.opt.grad_norm_clip_value)` and `EMA(Adam).step()` in one fused
        update.  Returns the 0-dim device loss; nothing is synchronised.  Keyword extensions `t_index`, `eta`, `seed` as `val_loss`.  The
        pieces stay available as `self.last_update`."""
        from .train import refuse_untrainable
        refuse_untrainable(self.model, condition, ldist.world()[1])
        return self._score_step(eps, None, cates, discrete, t_index, eta, seed)

    def _score_step(self, eps, condition, cates, discrete, t_index, eta, seed):
        """The body of `update_score` after the refusals.  condition: None, or the embedded (pts_condition, img_condition) pair
        (`CompletionTrainer`): the step then keeps the gradient with respect to that pair as `self.last_condition_grad`."""
        from . import ops
        from .train import ScoreTrainStep
        if not torch.is_tensor(eps) or not eps.is_cuda:
            raise RuntimeError("Trainer.update_score: eps is on %s; the HIP path has no CPU fallback"
                               % (eps.device if torch.is_tensor(eps) else type(eps).__name__,))
        self.warm_up(self.optimizer, self.itr)
        eps = eps.detach().float().contiguous()
        self.model.train()
        self.optimizer.zero_grad()
        t, e2int_f, var, weight_p = self._draw_times(eps.shape[0], discrete, "update_score", t_index=t_index,
                                                     iw_mode=None if discrete else self.cfg.sde.iw_sample_p_mode)
        if weight_p is not None:
            weight_p = weight_p.reshape(-1).float().to(eps.device)
        t_dev, xt, eta = self._diffuse(eps, t, e2int_f, var, eta, seed)
        if condition is None:
            step = ScoreTrainStep(self.model)
            params = step.forward(xt, t_dev, label=cates)
        else:
            step = ScoreTrainStep(self.model, allow_condition=True)
            params = step.forward(xt, t_dev, label=cates, condition=condition)
        l1 = self.cfg.opt.loss_type == "l1"
        loss, per_sample = ops.dsm_loss(eta, params, weight_p, l1=l1)
        dcondition = step.backward(ops.dsm_loss_bwd(eta, params, weight_p, l1=l1))
        if condition is not None:
            self.last_condition_grad = dcondition
        self.optimizer.step(max_norm=getattr(self.cfg.opt, "grad_norm_clip_value", None))
        self.model.invalidate_packed()                   # the update wrote the weights through raw pointers: no version counter moved
        self.last_update = {"t": t_dev, "eta": eta, "xt": xt, "params": params, "sample_loss": per_sample, "weight_p": weight_p,
                            "grad_norm": self.optimizer.last_norm, "lr": self.optimizer.param_groups[0]["lr"]}
        return loss

    def save(self, **kwargs):
        """The reference's checkpoint dict (:228-239) at `<cfg.log.save_path>/checkpt_<epoch>.pth`."""
        path = evalloop.checkpoint_path(self.cfg, self.epoch)
        torch.save({"cfg": self.cfg, "score_state_dict": self.model.state_dict(), "score_optim_state_dict": self.optimizer.state_dict(),
                    "score_scheduler": self.scheduler.state_dict(), "compressor_state_dict": self.compressor.state_dict(),
                    "epoch": self.epoch, "itr": self.itr, "time": self.time}, path)
        return path

    # ---- checkpoints: the reference's dict layout (:228-266) ------------------------------------------
    def resume(self, epoch=None, strict=False, load_optim=True, finetune=False, pretrain=None, **kwargs):
        """Same arguments as the reference (:241-266): the file is `pretrain` if given, else
        `<cfg.log.save_path>/checkpt_<epoch>.pth` with `epoch` defaulting to the last row of `training.csv`.
        (A path string passed as `epoch` is accepted as shorthand for `pretrain=`.)  Loads both state dicts, the
        optimizer's state — step, moments and the per-parameter 'ema' tensors — unless finetune / load_optim=False,
        and re-runs `compressor.init()`."""
        if finetune:
            load_optim, strict = False, False
        if isinstance(epoch, (str, os.PathLike)):
            pretrain, epoch = epoch, None
        if pretrain is None:
            pretrain = evalloop.checkpoint_path(self.cfg, epoch)
        ckpt = torch.load(pretrain, map_location="cpu", weights_only=False)   # holds cfg as argparse.Namespace
        self.model.load_state_dict(ckpt["score_state_dict"], strict=strict)
        self.compressor.load_state_dict(ckpt["compressor_state_dict"], strict=strict)
        self.compressor.init()
        if load_optim:
            osd = ckpt["score_optim_state_dict"]
            groups = osd.get("param_groups") or []
            if len(groups) == 1 and len(groups[0].get("params", ())) == len(self.optimizer.params):
                self.optimizer.load_state_dict(osd)              # :259 — step, both moments and the EMA of every parameter
            else:                                                # a state dict without Adam's groups: its 'ema' tensors only
                self.optimizer.load_ema(osd)
        if finetune:
            self.epoch, self.itr = 1, 0
        else:
            self.epoch, self.itr = ckpt["epoch"] + 1, ckpt["itr"]
        self.time = ckpt["time"]

    def load_pretrain(self, path=None):
        """Stage-1 compressor checkpoint (:268-273): key `state_dict`, strict."""
        path = self.cfg.compressor.pretrain_path if path is None else path
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        self.compressor.load_state_dict(ckpt["state_dict"], strict=True)
        self.compressor.init()


class CompletionTrainer(Trainer):
    """completion_trainer/Latent_SDE_Trainer.py (ShapeNet-ViPC completion, BASELINE configs[4]):
    `sample(num_samples, condition={'img': views, 'pts': partial})` runs the score model's ConditionNet once per call
    (:150-151; needs cfg.score.condition = True), samples image/partial-cloud conditioned latents and returns the decoded
    clouds only (:168); `valsample` is the evaluation loop of :170-215 without the dataset and the renderer.

    Training (:99-145): `update(data, condition)` / `update_score(eps, condition, ...)` take the EMBEDDED pair
    `(pts_condition (B, hidden, S), img_condition (B, t_dim) or 0.)` — what `model.c_net(...)` returns — and train the Score on it: the
    even blocks cross-attend to the condition tokens (ldt_attention_bwd_cross).  ConditionNet's own backward is not on this path: the
    gradient with respect to the pair is kept as `self.last_condition_grad = (d_pts_condition (B, hidden, S), d_img_condition (B, t_dim) or
    None)`, where that backward would start, and the `c_net` parameters of a `cfg.score.condition=True` model receive a zero gradient."""

    last_condition_grad = None

    def _refuse_condition(self, condition, who):
        """Everything this trainer's step does not take, each with its reason, before anything is launched or allocated."""
        from .train import refuse_untrainable
        if condition is None:
            raise NotImplementedError("CompletionTrainer.%s: this trainer's step trains on a ViPC / point condition and takes the embedded "
                                      "(pts_condition, img_condition) pair as `condition`; an unconditional step is Trainer.%s" % (who, who))
        refuse_untrainable(self.model, condition, ldist.world()[1], allow_condition=True)
        if not isinstance(condition, (tuple, list)) or len(condition) != 2:
            raise TypeError("CompletionTrainer.%s: condition is the pair (pts_condition, img_condition), got %s" % (who, type(condition).__name__))
        wd = max(float(g.get("weight_decay", 0.) or 0.) for g in self.optimizer.param_groups)
        if hasattr(self.model, "c_net") and wd != 0:
            raise NotImplementedError("CompletionTrainer.%s: weight_decay=%g with a ConditionNet in the model (cfg.score.condition=True) is not on "
                                      "this path: ConditionNet's backward is missing, its parameters receive a zero gradient, and a frozen "
                                      "net would silently decay" % (who, wd))

    def update(self, data, condition=None):
        """The reference's `update` (:99-111): `Trainer._update` on `data` (a tensor as upstream; a dict with `tr_points` is accepted too)
        without labels, with cfg.opt.discrete (default True).  Returns the 0-dim device loss."""
        self._refuse_condition(condition, "update")
        self._refuse_host("CompletionTrainer.update")
        return self._update(None, data["tr_points"] if isinstance(data, dict) else data, getattr(self.cfg.opt, "discrete", True), condition)

    def update_score(self, eps, condition=None, cates=None, discrete=True, *, t_index=None, eta=None, seed=None):
        """The reference's `update_score` (:113-145) with a condition pair: `Trainer.update_score`'s step (warm-up, times, `xt`, the loss,
        clip, EMA(Adam).step(); the keyword extensions mean the same) with the Score run as `model(xt, t, condition=condition,
        label=cates)`: with both a label and a condition the image condition is dropped (score.py:135)."""
        self._refuse_condition(condition, "update_score")
        return self._score_step(eps, tuple(condition), cates, discrete, t_index, eta, seed)

    @torch.no_grad()
    def sample(self, num_samples, num_points=None, label=None, condition=None, **kw):
        if isinstance(condition, dict):
            if not hasattr(self.model, "c_net"):
                raise ValueError("a raw condition dict needs cfg.score.condition=True (ConditionNet, score.py:64-65)")
            condition = self.model.c_net({k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in condition.items()})
        return super().sample(num_samples, num_points=num_points, label=label, condition=condition, **kw)[0]

    @torch.no_grad()
    def valsample(self, test_loader, vis=False, full=False, save_npy=None):
        """test_loader yields (views (B,3,H,W), pc (B,N,3), pc_part (B,Np,3)); both clouds are reduced to 2048 points by
        farthest point sampling (:181-184), the partial cloud + views condition the sampler, and L2_ChamferEval_1000 /
        F1Score over everything sampled are reported as upstream (:197-201).  full=False stops once more than 1000 shapes
        are accumulated (:203-205).  The `part_ep / smp_ep / ref_ep<epoch>.npy` dumps of :216-227 are written when
        cfg.log.save_path is set (save_npy=None) or on request (save_npy=True).  vis=True (mitsuba rendering, :208-213) is
        out of scope and raises.  Returns {'cd', 'f1', 'f1score', 'rate', 'samples', 'refs', 'parts'}."""
        import numpy as np
        from . import ops
        from .metrics import F1Score, L2_ChamferEval_1000
        evalloop.refuse_vis("valsample", vis)
        self.model.eval(); self.compressor.eval()
        all_ref, all_smp, all_part, use_time, count = [], [], [], 0., 0
        for views, pc, pc_part in test_loader:
            pc, pc_part = pc.to(self.device).float().contiguous(), pc_part.to(self.device).float().contiguous()
            ref_pts = ops.gather_rows(pc, ops.fps(pc, min(2048, pc.shape[1])))
            part = ops.gather_rows(pc_part, ops.fps(pc_part, min(2048, pc_part.shape[1])))
            _sync(self.device)
            t0 = time.time()
            smp = self.sample(num_samples=ref_pts.size(0), condition={"img": views.float(), "pts": part})
            _sync(self.device)
            use_time += time.time() - t0
            all_smp.append(smp); all_ref.append(ref_pts); all_part.append(part)
            count += smp.shape[0]
            if not full and count > 1000:                                             # :203-205
                break
        smp, ref, part = torch.cat(all_smp, 0), torch.cat(all_ref, 0), torch.cat(all_part, 0)
        cd = L2_ChamferEval_1000(smp, ref)
        f1, _, _ = F1Score(smp, ref)
        path = getattr(self.cfg.log, "save_path", "")
        if save_npy or (save_npy is None and path):
            for tag, t in (("part", part), ("smp", smp), ("ref", ref)):
                np.save(os.path.join(path, "%s_ep%d.npy" % (tag, self.epoch)), t.detach().cpu().numpy())
        print("Validation Sample (unit) Epoch:%d " % self.epoch, {"cd": float(cd), "f1score": float(f1.mean())})
        return {"cd": float(cd), "f1": float(f1.mean()), "f1score": float(f1.mean()), "rate": smp.shape[0] / max(use_time, 1e-9),
                "samples": smp, "refs": ref, "parts": part}


def _rows(t, lo, hi, per):
    """Rows [lo,hi) of a full-batch tensor, zero-padded to `per` rows (last rank when B % world != 0)."""
    part = t[lo:min(hi, t.shape[0])]
    if part.shape[0] < per:
        pad = torch.zeros((per - part.shape[0],) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
        part = torch.cat([part, pad], 0)
    return part
