"""`HybridTrainer` — the evaluation half of the reference's third trainer (trainer/Hybrid_Trainer.py; entry script train_Hybrid.py,
`--evaluate True` -> `valsample`; shipped config experiments/Hybrid_Trainer/airplane/config.yaml), MI355X path.

The hybrid trainer trains the Compressor and the Score together, LSGM style: the Compressor's KL term is measured against the diffusion
prior instead of N(0, 1).  Kept, with the reference's names, signatures and return values: `Trainer(cfg, model, compressor, device)`
(:23-61), `score_fn` (:63-67), `sample` (:162-185; the points only), `valsample` (:187-247), `valrecon` (:249-308), `resume` /
`load_pretrain` (:325-357).  New: `val_nelbo`, the forward terms of `clc_compressor` (:117-143) on held-out data — the latent NELBO,
    kl = mean(log q(z) - log p(z)),   log p(z) = -(|eta - eps_theta(x_t, t)|^2 w_q(t) + c),   c = 1/2 (1 + log(2 pi var(time_eps))),
with t drawn by `DiffusionBase.iw_quantities` (or from the discrete grid).  Training is out of scope: there is no optimizer, and `update`,
`update_score`, `clc_compressor` and `save` raise.  The hybrid config's Score alone does train: through
`ldt_amd.Trainer.update_score(eps, discrete=True)` on latents from a frozen Compressor (the reference's hybrid `update_score`, :88-113, with
`weight_p` = 1).

The encode, x_t, the Score forward, the two sums of the KL term (ldt_nelbo_terms), Chamfer, the samplers and the decode run in HIP
kernels; what is plain torch here is bookkeeping on finished tensors and on (B,) host schedules.
"""
import os
import time

import torch

from . import dist as ldist
from . import evalloop, ops
from .evalloop import _sync
from .trainer import Trainer


def _not_trained(name):
    return NotImplementedError("HybridTrainer.%s: training (backward pass, optimizer step) is not on this path — it is the inference / "
                               "evaluation path; val_nelbo returns the forward terms of clc_compressor on held-out data" % name)


class HybridTrainer(Trainer):
    def __init__(self, cfg, model, compressor, device):
        if cfg.sde.sde_type not in ("vpsde", "sub_vpsde", "vesde"):               # Hybrid_Trainer.py:25-32
            raise TypeError("cfg.sde.sde_type %r: 'vpsde', 'sub_vpsde' or 'vesde'" % (cfg.sde.sde_type,))
        super().__init__(cfg, model, compressor, device)                           # SDE, models, EMAWeights, sampling fields, epoch / itr / time
        self.ode_tol = cfg.sde.ode_tol
        self.compressor_warmup = getattr(cfg.opt, "compressor_warmup", None)      # (training only: read when present)
        self.alpha = getattr(cfg.opt, "alpha", None)
        self.N = cfg.sde.train_N
        self.discrete = cfg.opt.discrete
        self.time_eps = cfg.sde.time_eps

    # ---- training: refused -------------------------------------------------------------------------------
    def update(self, data, condition=None, train_individual=True):
        raise _not_trained("update")

    def update_score(self, eps, condition=None, cates=None):
        raise _not_trained("update_score")

    def clc_compressor(self, point, cates=None, condition=None, discrete=False, train_score=True):
        raise _not_trained("clc_compressor")

    def save(self, **kwargs):
        raise _not_trained("save")

    # ---- held-out latent NELBO ---------------------------------------------------------------------------------
    @torch.no_grad()
    def val_nelbo(self, data, condition=None, *, discrete=None, rho=None, t_index=None, eta=None, post_noise=None, seed=None):
        """The forward terms of `clc_compressor` (Hybrid_Trainer.py:117-143) for one held-out batch, inside `Trainer._ema_weights`:
          1. `compressor(data['te_points'], want_kl=True)`: `all_eps`, the reconstruction, the per-level log q(z);
          2. log q(z) concatenated to the layout of `all_eps` (:119);
          3. the times (`Trainer._draw_times`) — `discrete` (default cfg.opt.discrete) True: the grid, and w_q = g2 / (2 var) (:122-127);
             False: cfg.sde.iw_sample_q_mode with its weight (:129-134);
          4. x_t and eta (`Trainer._diffuse`), as in `Trainer.val_loss`;
          5. `Score(x_t, t, label=, condition=)` with the per-sample times, label from `data['cate_idx']` when cfg.data.num_categorys > 1;
          6. c = 1/2 (1 + log(2 pi var(time_eps))) (:140-141), and the two sums of kl in one pass (ldt_nelbo_terms).
        Returns 0-dim device tensors {'kl': mean(logqz - logpz), 'logqz': mean log q(z), 'score_term': mean |eta - params|^2 w_q,
        'cross_entropy_const': c, 'rec_cd': the Chamfer term of `CompressorTrainer.eval_losses` (CD_loss 'l1')}; nothing is synchronised.
        The auction-EMD term of upstream's `rec_loss` is absent for the reason `CompressorTrainer.compute_loss` gives.

        Both models are in eval mode.  Upstream calls `compressor.train()` at this point because it is about to take a gradient step;
        the HIP path folds BatchNorm's running statistics into its weights and is an evaluation path, so the held-out figure is the
        eval-mode one.

        Keyword extensions (not in the reference): `rho` (B,) replaces the uniform draw of `iw_quantities`, `t_index` (B,) the numpy
        draw of the discrete branch, `eta` (B, tokens, z) the diffusion noise, `post_noise` the Compressor's posterior noise (a list of
        n_layers (B, tokens, z_dim) tensors), `seed` the Philox key of eta.  The pieces stay available as `self.last_val_nelbo`."""
        self.model.eval()
        self.compressor.eval()
        with self._ema_weights():
            dev = self.device
            target = data["te_points"].to(dev).float().contiguous()
            kw = {} if post_noise is None else {"post_noise": post_noise}
            out = self.compressor(target, want_kl=True, **kw)
            eps = out["all_eps"]
            logqz = torch.cat(out["all_logqz"], dim=1).transpose(1, 2).contiguous()        # (B, tokens, n_layers * z): all_eps's layout
            label = self._label(data)
            size = eps.shape[0]
            discrete = self.discrete if discrete is None else discrete
            t, e2int_f, var, weight_q = self._draw_times(size, discrete, "val_nelbo", t_index=t_index, rho=rho,
                                                         iw_mode=None if discrete else self.cfg.sde.iw_sample_q_mode)
            if discrete:
                weight_q = self.SDE.g2(t) / (2 * var)                                      # (:122-127: the NELBO's weight on the grid)
            weight_q = weight_q.reshape(-1).float().expand(size).contiguous()              # ((1, 1) under 'drop_all_uniform')
            t_dev, xt, eta = self._diffuse(eps, t, e2int_f, var, eta, seed)
            params = self.model(xt, t_dev, condition=condition, label=label)
            w_dev = weight_q.to(dev)
            sums, per_sample = ops.nelbo_terms(eta, params, logqz, w_dev)
            c = self.SDE.cross_entropy_const(self.time_eps).to(dev)
            n = float(eps.numel())
            d_rec, d_tgt = ops.chamfer(target, out["set"].contiguous())
            res = {"kl": (sums[0] + sums[1]) / n + c, "logqz": sums[1] / n, "score_term": sums[0] / n, "cross_entropy_const": c,
                   "rec_cd": torch.sqrt(d_rec.clamp_min(0)).mean() + torch.sqrt(d_tgt.clamp_min(0)).mean()}
            self.last_val_nelbo = dict(res, t=t_dev, weight_q=w_dev, var=var, e2int_f=e2int_f, eps=eps, logqz=logqz, eta=eta, xt=xt,
                                       params=params, set=out["set"], sample_sums=per_sample, batch_sums=sums)
        return res

    # ---- generation ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, num_samples, label=None, condition=None, *, num_points=None, x0=None, noise=None, seed=None, use_graph=None,
               trajectory=None):
        """:162-185 — `Trainer.sample` (both sample modes, EMA swap, sharding, `LDT_ODE_SOLVER`) returning the decoded points only
        (survey quirk Q12), with upstream's `NFE:..., NFEs.../s` print (:182; the clock here covers the decode too and is read after the
        device has finished).  The sampled latents stay available as `self.last_eps`."""
        _sync(self.device)
        t0 = time.time()
        pts, self.last_eps = super().sample(num_samples, num_points=num_points, label=label, condition=condition, x0=x0, noise=noise,
                                            seed=seed, use_graph=use_graph, trajectory=trajectory)
        _sync(self.device)
        nfe_count = self.nfe_count if self.sample_mode == "continuous" else self.cfg.sde.sample_N
        if ldist.world()[0] == 0:
            print('NFE:{:}, NFEs{:.2f}/s'.format(nfe_count, nfe_count / max(time.time() - t0, 1e-9)))
        return pts

    @torch.no_grad()
    def valsample(self, test_loader, val_cate=0, vis=False):
        """:187-247, upstream's behaviour kept: `Trainer.valsample`'s references and sampled batches (evalloop.collect_refs / sample_clouds),
        the label-conditioned ones NOT cut to len(ref) (:223-224).  The "Sample rate" print on every rank, the dump on rank 0 under
        upstream's literal name 'smp{:}_ep<epoch>.npy' (:228 fills only the %d), `compute_all_metrics(smp, ref, batch_size=64)` and its
        report.  vis=True (mitsuba) raises."""
        evalloop.refuse_vis("valsample", vis)
        from .metrics import compute_all_metrics
        self.model.eval()
        self.compressor.eval()
        dev, d = self.device, self.cfg.data
        cate = None if d.num_categorys == 1 else val_cate
        ref, sizes, _ = evalloop.collect_refs(test_loader, dev, "valsample", cate, None if cate is None else d.test_batch_size)
        smp, use_time = evalloop.sample_clouds(self.sample, sizes, dev, cate)
        print("Sample rate: %.8f " % (smp.shape[0] / max(use_time, 1e-9)))
        self.last_valsample = {"samples": smp, "refs": ref}
        evalloop.dump(self.cfg, 'smp{:}_ep%d' % self.epoch + ".npy", smp, ldist.world()[0] == 0)
        return evalloop.report(self.epoch, compute_all_metrics(smp, ref, batch_size=64))

    @torch.no_grad()
    def valrecon(self, test_loader, val_cate=0, *args, **kwargs):
        """:249-308 — `evalloop.reconstruct` with the Compressor, without a label, the by-category branch de-normalised by `mean` / `std`;
        then the `rec_ep<epoch>.npy` dump (rank 0) and `compute_all_metrics(rec, ref, batch_size=256)`.
        Upstream's single-category branch calls `self.model(ref_pts)` (:261) — the Score on a point cloud — and cannot run; what is meant,
        and what the other branch does (:289), is `self.compressor(ref_pts)`, which is what runs here."""
        from .metrics import compute_all_metrics
        self.model.eval()
        self.compressor.eval()
        rec, ref = evalloop.reconstruct(self.compressor, test_loader, self.cfg, self.device, val_cate, "valrecon",
                                        fields=("mean", "std"), with_label=False)
        self.last_valrecon = {"rec": rec, "ref": ref}
        evalloop.dump(self.cfg, 'rec_ep%d' % self.epoch + ".npy", rec, ldist.world()[0] == 0)
        return evalloop.report(self.epoch, compute_all_metrics(rec, ref, batch_size=256))

    # ---- checkpoints: the dict `save` writes upstream (:310-323) -------------------------------------------------
    def resume(self, epoch=None, strict=False, load_optim=True, finetune=False, *, pretrain=None, **kwargs):
        """:325-350 — `<cfg.log.save_path>/checkpt_<epoch>.pth` (`epoch` defaults to the last row of `training.csv`; keyword extension
        `pretrain`: that file instead): `score_state_dict`, `compressor_state_dict`, `compressor.init()`; with `load_optim` the EMA tensors
        of `score_optim_state_dict`; `epoch` (+ 1), `itr` (1 and 0 under `finetune`) and `time`.  `score_scheduler`,
        `compressor_optim_state_dict` and `compressor_scheduler` are read past: there is no optimizer here."""
        super().resume(epoch=epoch, strict=strict, load_optim=load_optim, finetune=finetune, pretrain=pretrain)

    def load_pretrain(self):
        """:352-357 — `cfg.opt.pretrain_path`, keys `score_state_dict` and `compressor_state_dict`, strict."""
        checkpt = torch.load(os.path.join(self.cfg.opt.pretrain_path), map_location="cpu", weights_only=False)
        self.model.load_state_dict(checkpt["score_state_dict"], strict=True)
        self.compressor.load_state_dict(checkpt["compressor_state_dict"], strict=True)
        self.compressor.init()
