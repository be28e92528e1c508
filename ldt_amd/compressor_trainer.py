"""`CompressorTrainer` / `CompletionCompressorTrainer` — the evaluation half of the reference's stage-1 trainers
(trainer/Compressor_Trainer.py, completion_trainer/Compressor_Trainer.py), MI355X path: what the `--test` branches of
train_Compressor.py (:72,99) and train_Completion_Compressor.py (:81,108) call.

Kept, with the reference's names, signatures and return values: `Trainer(cfg, model, device)`, `sample` (:54-59), `valsample`
(:61-100), `reconstrustion` (:102-161; completion :66-95 — upstream's spelling), `resume` (:163-186).  New: `eval_losses`, the two
ELBO terms of `compute_loss` that need no absent extension, and `update_decoder`, one training step of the DECODER with the encoder
frozen (compressor_train.DecoderTrainStep, losses.cd_loss): the Chamfer reconstruction loss, the top-down backward,
Adam without EMA over the decoder-side parameters, and the gradient with respect to the latents kept as `last_eps_grad`; and
`update_topdown`, one step of the whole top-down half — posterior blocks, prior heads, the reparameterised draw and the KL term, then the
decoder — with the bottom-up half frozen (compressor_train.TopDownTrainStep; section 4.16): loss = kl_weight * kl_loss + the Chamfer term,
the gradient with respect to the encoder outputs kept as `last_enc_out_grad`; and `update_encoder`, that step with ActNorm and the encoder
in the graph and only the front (input conv, grouper, position embedding) frozen (compressor_train.EncoderTrainStep; section 4.17), the
gradients with respect to the grouped tokens and the position condition kept as `last_tokens_grad` / `last_pos_grad`; and `update_front`,
that step with the front in the graph too, in training mode for its BatchNorms (compressor_train.FrontTrainStep; section 4.19): every
parameter of the Compressor receives a gradient.  The reference's own step stays out of scope: `update` / `compute_loss` raise —
`compute_loss` adds `EMD_loss`, which goes through the auction-EMD CUDA extension of evaluation/emd.py that this package does not have
(and does not imitate).

The encode, the decode, Chamfer / EMD and the KL terms run in HIP kernels (Compressor.forward, ldt_amd.metrics); the bookkeeping on
finished clouds — concatenation, the loaders' shift / scale de-normalisation, the category filter, report and dump — is ldt_amd/evalloop.py's,
shared with the two Score trainers.
"""
import os

import torch

from . import evalloop, ops
from .metrics import F1Score, L2_ChamferEval_1000, compute_all_metrics


class CompressorTrainer:
    def __init__(self, cfg, model, device):
        self.cfg = cfg
        self.device = device
        self.itr, self.epoch, self.time = 0, 1, 0                    # trainer/base.py:20-26
        self.num_points = cfg.data.tr_max_sample_points
        self.kl_weight = getattr(cfg.opt, "kl_weight", None)
        self.model = model.to(device)

    # ---- training: refused -------------------------------------------------------------------------------
    def update(self, data):
        raise NotImplementedError("CompressorTrainer.update: training (optimizer step, backward) is not on this path — it is the "
                                  "inference / evaluation path; see eval_losses for the held-out KL and Chamfer terms")

    def compute_loss(self, target_set, label):
        raise NotImplementedError("CompressorTrainer.compute_loss: its EMD_loss term needs the auction-EMD CUDA extension "
                                  "(evaluation/emd.py), which is not on this path; eval_losses returns the KL and Chamfer terms")

    # ---- training the decoder with the encoder frozen ---------------------------------------------------
    optimizer = None                                                 # AdamEMA over the decoder-side parameters, created by the first update_decoder
    last_eps_grad = None                                             # d loss / d eps of the last update_decoder

    def warm_up(self, optimizer, itr):
        evalloop.warm_up(self.cfg, optimizer, itr)

    # ---- what the three update_* steps share ------------------------------------------------------------------
    def _points(self, who, data):
        """The device refusal, then data['tr_points'] (or the tensor itself) as fp32 on the device."""
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("CompressorTrainer.%s: device %s; the HIP path has no CPU fallback" % (who, self.device))
        return (data["tr_points"] if isinstance(data, dict) else data).to(self.device).float().contiguous()

    def _frozen(self, part):
        """part() under no_grad with the model in evaluation mode: a frozen part runs as in evaluation; the caller's mode comes back."""
        was_training = self.model.training
        try:
            with torch.no_grad():
                self.model.eval()
                return part()
        finally:
            self.model.train(was_training)

    def _draws(self, B, N, T, post_noise):
        """-> (keep_mask, post_noise) in the order of Compressor.forward on the CPU generator: InitialSet's row subsets, then the posterior
        draws (unless given)."""
        m = self.model
        keep_mask = m._presence(B, N)
        if keep_mask is None:                                        # (every row kept: said so, so that the step does not draw again)
            keep_mask = torch.ones((B, m.max_outputs), dtype=torch.bool)
        if post_noise is None:
            if m.reference_rng:
                post_noise = [torch.randn((B, m.z_dim, T)).transpose(1, 2).to(self.device) for _ in range(m.n_layers)]
            else:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                post_noise = [ops.philox_normal((B, T, m.z_dim), torch.device(self.device), seed, step=j) for j in range(m.n_layers)]
        return keep_mask, post_noise

    def _begin(self, attr, parameters):
        """The optimizer kept as `self.<attr>` (Adam without EMA over parameters(), created at its first use), warmed up and zeroed."""
        if getattr(self, attr) is None:
            from .train import AdamEMA
            o = self.cfg.opt
            setattr(self, attr, AdamEMA([p for _, p in parameters()], lr=o.lr, betas=(o.beta1, o.beta2), weight_decay=o.weight_decay, ema_decay=0.))
        optimizer = getattr(self, attr)
        self.warm_up(optimizer, self.itr)
        optimizer.zero_grad()
        return optimizer

    def _finish(self, optimizer):
        optimizer.step(max_norm=getattr(self.cfg.opt, "grad_norm_clip_value", None))
        self.model.invalidate_packed()                               # the update wrote the weights through raw pointers
        self.itr += 1

    def _topdown_pass(self, points, enc_out, post_noise, keep_mask, T):
        """The top-down forward with its tape, loss = kl_weight * kl_loss + `CD_loss(set, points)` of type 'l1', and the interleaved backward
        with kl_scale = kl_weight / numel(cat(kls)) -> ((loss, kl_loss, rec_loss), d_enc_out)."""
        from .compressor_train import TopDownTrainStep
        from .losses import cd_loss
        m = self.model
        step = TopDownTrainStep(m)
        out, _, kl_sample_sum = step.forward([t.to(self.device) for t in enc_out], [t.to(self.device) for t in post_noise],
                                             num_points=points.shape[1], keep_mask=keep_mask)
        n_kl = m.n_layers * points.shape[0] * m.z_dim * T            # numel(torch.cat(kls, dim=1))
        kl_loss = kl_sample_sum.sum() / n_kl
        rec_loss, d_set = cd_loss(out, points, "l1", want_grad=True)
        d_enc_out = step.backward(d_set, self.kl_weight / n_kl)
        return (self.kl_weight * kl_loss + rec_loss, kl_loss, rec_loss), d_enc_out

    def update_decoder(self, data, *, eps=None, post_noise=None):
        """One training step of the decoder with the encoder frozen: eps = model.encode(data['tr_points']) under no_grad (or `eps` as
        given; `post_noise` replaces the posterior draws), the learning-rate warm-up, the top-down decode with its tape
        (compressor_train.DecoderTrainStep), the Chamfer reconstruction loss `CD_loss(set, points)` of type 'l1' with its gradient
        (ldt_amd.losses.cd_loss), the backward, clip_grad_norm_(cfg.opt.grad_norm_clip_value) and Adam(lr, (beta1, beta2), weight_decay) —
        the reference's stage-1 optimizer has no EMA — over the decoder-side parameters, `itr += 1`.  -> (loss, rec_loss), 0-dim device
        tensors: with the encoder frozen the KL term has no gradient on this side, and the EMD term stays absent (compute_loss), so the
        loss IS the Chamfer term.  `self.last_eps_grad` keeps d loss / d eps (B, tokens, n_layers * z_dim), where the posterior / encoder
        backward would start."""
        from .compressor_train import DecoderTrainStep, decoder_parameters, refuse_undecodable
        from .losses import cd_loss
        refuse_undecodable(self.model)
        points = self._points("update_decoder", data)
        if eps is None:
            eps = self._frozen(lambda: self.model.encode(points, post_noise=post_noise))
        optimizer = self._begin("optimizer", lambda: decoder_parameters(self.model))
        step = DecoderTrainStep(self.model)
        out = step.forward(eps.to(self.device), num_points=points.shape[1])
        loss, d_set = cd_loss(out, points, "l1", want_grad=True)
        self.last_eps_grad = step.backward(d_set)
        self._finish(optimizer)
        return loss, loss

    # ---- training the top-down half with the bottom-up half frozen -------------------------------------------
    topdown_optimizer = None                                         # AdamEMA over the top-down parameters, created by the first update_topdown
    last_enc_out_grad = None                                         # d loss / d (encoder outputs) of the last update_topdown

    def update_topdown(self, data, *, enc_out=None, post_noise=None):
        """One training step of the top-down half (posterior blocks, prior heads, decoder; compressor_train.TopDownTrainStep, DESIGN.md
        section 4.16) with the bottom-up half frozen: the encoder outputs from `model.bottom_up(data['tr_points'])` under no_grad in
        evaluation mode (or `enc_out`, n_layers tensors (B, tokens, hidden), as given), the posterior draws as `Compressor.forward` draws
        them (or `post_noise`), the learning-rate warm-up, the top-down pass with its tape, `CD_loss(set, points)` of type 'l1' with its
        gradient, the interleaved backward with kl_scale = kl_weight / numel(cat(kls)), clip_grad_norm_ and Adam without EMA over the
        top-down parameters (`self.topdown_optimizer`, apart from update_decoder's), `itr += 1`.  -> (loss, kl_loss, rec_loss), 0-dim
        device tensors as the reference's `update` returns them: loss = kl_weight * kl_loss + rec_loss with kl_loss formed as
        eval_losses forms it.  The reference's rec_loss also holds EMD_loss, which is absent here (compute_loss says why): rec_loss IS the
        Chamfer term.  `self.last_enc_out_grad` keeps d loss / d enc_out, where the encoder backward would start."""
        from .compressor_train import refuse_untrainable_topdown, topdown_parameters
        if self.kl_weight is None:
            raise ValueError("CompressorTrainer.update_topdown: cfg.opt.kl_weight is not set; the loss is kl_weight * kl_loss + rec_loss")
        refuse_untrainable_topdown(self.model)
        m = self.model
        points = self._points("update_topdown", data)
        if enc_out is None:
            T = m.z_scales
            enc_out = self._frozen(lambda: [o.transpose(1, 2) for o in m.bottom_up(points)["outputs"]])
        else:
            T = enc_out[0].shape[1]
        keep_mask, post_noise = self._draws(points.shape[0], points.shape[1], T, post_noise)
        optimizer = self._begin("topdown_optimizer", lambda: topdown_parameters(m))
        losses, self.last_enc_out_grad = self._topdown_pass(points, enc_out, post_noise, keep_mask, T)
        self._finish(optimizer)
        return losses

    # ---- training the encoder and the top-down half with the grouped tokens frozen ---------------------------
    encoder_optimizer = None                                         # AdamEMA over the encoder + top-down parameters, created by the first update_encoder
    last_tokens_grad = None                                          # d loss / d tokens (before ActNorm) of the last update_encoder
    last_pos_grad = None                                             # d loss / d (position condition) of the last update_encoder

    def update_encoder(self, data, *, tokens=None, pos=None, post_noise=None):
        """`update_topdown` with the encoder in the graph (compressor_train.EncoderTrainStep): the grouped tokens and
        the position condition from `model.front(data['tr_points'])` under no_grad in evaluation mode (or `tokens` (B, T, hidden) before
        ActNorm and `pos` (B, p_dim) as given) stay frozen; ActNorm and the encoder stages run with their tape, the top-down pass on their
        outputs, `CD_loss` of type 'l1', the interleaved top-down backward and, from its d_enc_out, the encoder backward.  While
        `model.conv_in.initialized` is 0 the reference's data-dependent ActNorm init runs first on these tokens (layers.py:74-79, 84-92:
        shift = the batch mean, log_scale = log(unbiased batch std + eps); torch on the device, once).  clip_grad_norm_ and Adam without EMA
        over the encoder + top-down parameters (`self.encoder_optimizer`, apart from the other two), `itr += 1`.  -> (loss, kl_loss,
        rec_loss) as update_topdown.  `self.last_tokens_grad` (B, T, hidden) and `self.last_pos_grad` (B, p_dim) keep what the grouper's
        and the position embedding's backward would start from."""
        from .compressor_train import (EncoderTrainStep, encoder_parameters, refuse_untrainable_encoder, refuse_untrainable_topdown,
                                       topdown_parameters)
        if self.kl_weight is None:
            raise ValueError("CompressorTrainer.update_encoder: cfg.opt.kl_weight is not set; the loss is kl_weight * kl_loss + rec_loss")
        refuse_untrainable_encoder(self.model)
        refuse_untrainable_topdown(self.model)
        m = self.model
        points = self._points("update_encoder", data)
        if tokens is None or pos is None:
            fr = self._frozen(lambda: m.front(points))
            tokens = fr["tokens"] if tokens is None else tokens
            pos = fr["pos"] if pos is None else pos
        tokens, pos = tokens.to(self.device).float().contiguous(), pos.to(self.device).float().contiguous()
        self._actnorm_data_init(tokens)
        keep_mask, post_noise = self._draws(points.shape[0], points.shape[1], tokens.shape[1], post_noise)
        optimizer = self._begin("encoder_optimizer", lambda: encoder_parameters(m) + topdown_parameters(m))
        enc = EncoderTrainStep(m)
        enc_out = enc.forward(tokens, pos)
        losses, d_enc_out = self._topdown_pass(points, enc_out, post_noise, keep_mask, tokens.shape[1])
        self.last_tokens_grad, self.last_pos_grad = enc.backward(d_enc_out)
        self._finish(optimizer)
        return losses

    def _actnorm_data_init(self, tokens):
        """While `model.conv_in.initialized` is 0: ActNorm.data_init (layers.py:74-79) on these tokens, torch on the device, once."""
        m = self.model
        if m.ActNorm is None or bool(m.conv_in.initialized):
            return
        with torch.no_grad():
            ci = m.conv_in
            x = tokens.view(-1, 1, tokens.shape[2]) if ci.feature_type == "set" else tokens
            ci.shift.data.copy_(torch.mean(x, dim=0, keepdim=True))
            ci.log_scale.data.copy_(torch.log(torch.std(x, dim=0, keepdim=True) + ci.eps))
            ci.initialized += 1.
        m.invalidate_packed()

    # ---- training the whole Compressor: the front in the graph too -------------------------------------------
    front_optimizer = None                                           # AdamEMA over every parameter, created by the first update_front

    def update_front(self, data, *, post_noise=None):
        """`update_encoder` with the front in the graph (compressor_train.FrontTrainStep), so that every parameter of
        the Compressor receives a gradient: the input conv, the grouper and the position embedding run on data['tr_points'] in TRAINING mode
        with their tape — every BatchNorm normalises with the batch statistics and updates its running buffers as nn.BatchNorm1d does — then
        the data-dependent ActNorm init (while `initialized` is 0), the draws, the encoder and the top-down pass, `CD_loss` of type 'l1', the
        three backwards in reverse, clip_grad_norm_ and Adam without EMA over all parameters (`self.front_optimizer`, apart from the other
        three), `itr += 1`.  -> (loss, kl_loss, rec_loss) as update_encoder: rec_loss IS the Chamfer term (compute_loss says why).
        `self.last_tokens_grad` / `self.last_pos_grad` keep what the front's backward started from."""
        from .compressor_train import (EncoderTrainStep, FrontTrainStep, encoder_parameters, front_parameters, refuse_untrainable_encoder,
                                       refuse_untrainable_front, refuse_untrainable_topdown, topdown_parameters)
        if self.kl_weight is None:
            raise ValueError("CompressorTrainer.update_front: cfg.opt.kl_weight is not set; the loss is kl_weight * kl_loss + rec_loss")
        m = self.model
        refuse_untrainable_front(m)
        refuse_untrainable_encoder(m)
        refuse_untrainable_topdown(m)
        points = self._points("update_front", data)
        front = FrontTrainStep(m)
        tokens, pos = front.forward(points)
        self._actnorm_data_init(tokens)
        keep_mask, post_noise = self._draws(points.shape[0], points.shape[1], tokens.shape[1], post_noise)
        optimizer = self._begin("front_optimizer", lambda: front_parameters(m) + encoder_parameters(m) + topdown_parameters(m))
        enc = EncoderTrainStep(m)
        enc_out = enc.forward(tokens, pos)
        losses, d_enc_out = self._topdown_pass(points, enc_out, post_noise, keep_mask, tokens.shape[1])
        self.last_tokens_grad, self.last_pos_grad = enc.backward(d_enc_out)
        front.backward(self.last_tokens_grad, self.last_pos_grad)
        self._finish(optimizer)
        return losses

    @torch.no_grad()
    def eval_losses(self, target_set, label=None):
        """The two terms of `compute_loss` (:42-52) that stand on kernels of this package, for a held-out batch (B, N, 3):
        'kl_loss' = `torch.cat(kls, dim=1).mean()` and 'cd_loss' = `CD_loss(output_set, target_set)` of evaluation/loss.py:72-79
        (type 'l1': mean sqrt(dist1) + mean sqrt(dist2), on ldt_chamfer).  0-dim device tensors."""
        self.model.eval()
        target = target_set.to(self.device).float().contiguous()
        out = self.model(target, label=label, want_kl=True)
        n_kl = sum(k.numel() for k in out["kls"])
        kl_loss = out["kl_sample_sum"].sum() / n_kl                  # the per-sample, per-level sums are the kernel's; every level is equally long
        d_rec, d_tgt = ops.chamfer(target, out["set"].contiguous())  # squared distances: reconstruction -> target, target -> reconstruction
        cd_loss = torch.sqrt(d_rec.clamp_min(0)).mean() + torch.sqrt(d_tgt.clamp_min(0)).mean()
        return {"kl_loss": kl_loss, "cd_loss": cd_loss}

    # ---- generation ------------------------------------------------------------------------------------------
    def sample(self, num_samples, num_points, given_eps=None):
        self.model.eval()
        with torch.no_grad():
            return self.model.sample((num_samples, num_points), given_eps=given_eps)

    @torch.no_grad()
    def valsample(self, test_loader, sample_points, vis=False):
        """:61-100 — one prior sample per test shape (latents ~ N(0, 1)), the "Sample rate" print, `smp_ep<epoch>.npy` into
        cfg.log.save_path (when one is set), `compute_all_metrics(smp, ref)` and the `{"val/gen/<key>": float}` dict."""
        evalloop.refuse_vis("valsample", vis)
        self.model.eval()
        ref, sizes, _ = evalloop.collect_refs(test_loader, self.device, "valsample")
        smp, use_time = evalloop.sample_clouds(lambda num_samples: self.sample(num_samples=num_samples, num_points=sample_points),
                                               sizes, self.device)
        print("Sample rate: %.8f " % (smp.shape[0] / max(use_time, 1e-9)))
        evalloop.dump(self.cfg, "smp_ep%d.npy" % self.epoch, smp)
        return evalloop.report(self.epoch, compute_all_metrics(smp, ref, batch_size=128))

    # ---- reconstruction ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def reconstrustion(self, test_loader, val_cate=0):
        """:102-161 — `evalloop.reconstruct` with the model, de-normalised by the loader's `shift` / `scale` in both branches, the
        by-category batches encoded with the label `val_cate`; then `rec_ep<epoch>.npy` and `compute_all_metrics(rec, ref,
        batch_size=128)`.  Nothing synchronises until the dump and the metrics at the end."""
        self.model.eval()
        rec, ref = evalloop.reconstruct(self.model, test_loader, self.cfg, self.device, val_cate, "reconstrustion",
                                        fields=("shift", "scale"), with_label=True)
        evalloop.dump(self.cfg, "rec_ep%d.npy" % self.epoch, rec)
        self.last_reconstruction = {"rec": rec, "ref": ref}
        return evalloop.report(self.epoch, compute_all_metrics(rec, ref, batch_size=128))

    # ---- checkpoints: the layout trainer/base.py:51-61 `save` writes ---------------------------------------------
    def resume(self, epoch=None, finetune=False, strict=False, load_optim=True):
        """:163-186 — `<cfg.log.save_path>/checkpt_<epoch>.pth` (`epoch` defaults to the last row of `training.csv`): the weights from
        `state_dict`; unless `finetune`, also `epoch` (+ 1), `itr` and `time`.  The optimizer and scheduler entries are ignored
        (`load_optim` is accepted for signature parity): there is no optimizer here.  Ends with `model.init()` like upstream."""
        path = evalloop.checkpoint_path(self.cfg, epoch)
        checkpt = torch.load(path, map_location="cpu", weights_only=False)      # holds cfg as argparse.Namespace
        if not finetune:
            self.model.load_state_dict(checkpt["state_dict"], strict=strict)
            self.epoch = checkpt["epoch"] + 1
            self.itr = checkpt["itr"]
            self.time = checkpt["time"]
        else:
            self.model.load_state_dict(checkpt["state_dict"], strict=False)
        self.model.init()


class CompletionCompressorTrainer(CompressorTrainer):
    """completion_trainer/Compressor_Trainer.py (ShapeNet-ViPC): same constructor, `sample` and `resume`; `reconstrustion` takes the
    ViPC loader's (views, pc, pc_part) batches and reports Chamfer / F1 instead of the generation metrics."""

    def update(self, data):
        raise NotImplementedError("CompletionCompressorTrainer.update: training (optimizer step, backward) is not on this path — it is "
                                  "the inference / evaluation path; see eval_losses for the held-out KL and Chamfer terms")

    def update_decoder(self, data, *, eps=None, post_noise=None):
        raise NotImplementedError("CompletionCompressorTrainer.update_decoder: the decoder step is built and held for CompressorTrainer "
                                  "alone; training is not on this path for the completion trainer")

    def update_topdown(self, data, *, enc_out=None, post_noise=None):
        raise NotImplementedError("CompletionCompressorTrainer.update_topdown: the top-down step is built and held for CompressorTrainer "
                                  "alone; training is not on this path for the completion trainer")

    def update_encoder(self, data, *, tokens=None, pos=None, post_noise=None):
        raise NotImplementedError("CompletionCompressorTrainer.update_encoder: the encoder step is built and held for CompressorTrainer "
                                  "alone; training is not on this path for the completion trainer")

    def update_front(self, data, *, post_noise=None):
        raise NotImplementedError("CompletionCompressorTrainer.update_front: the front step is built and held for CompressorTrainer "
                                  "alone; training is not on this path for the completion trainer")

    def compute_loss(self, target_set):
        raise NotImplementedError("CompletionCompressorTrainer.compute_loss: its EMD_loss term needs the auction-EMD CUDA extension "
                                  "(evaluation/emd.py), which is not on this path; eval_losses returns the KL and Chamfer terms")

    @torch.no_grad()
    def reconstrustion(self, test_loader):
        """:66-95 — every complete cloud reduced to 2048 points by farthest point sampling, encoded and reconstructed;
        `rec_ep<epoch>.npy`; returns {'cd': L2_ChamferEval_1000(rec, ref), 'f1score': F1Score(rec, ref).mean()}."""
        self.model.eval()
        all_ref, all_rec = [], []
        for views, pc, pc_part in test_loader:
            pc = pc.to(self.device).float().contiguous()
            ref_pts = ops.gather_rows(pc, ops.fps(pc, min(2048, pc.shape[1])))
            all_rec.append(self.model(ref_pts)["set"])
            all_ref.append(ref_pts)
        rec, ref = torch.cat(all_rec, dim=0), torch.cat(all_ref, dim=0)
        evalloop.dump(self.cfg, "rec_ep%d.npy" % self.epoch, rec)
        self.last_reconstruction = {"rec": rec, "ref": ref}
        cd =L2_ChamferEval_1000(rec, ref)
        f1score, _, _ = F1Score(rec, ref)
        all_res = {"cd": cd, "f1score": f1score.mean()}
        print("Validation Sample (unit) Epoch:%d " % self.epoch, all_res)
        return all_res

    def load_pretrain(self):
        """:122-126 — `cfg.model.pretrain_path`, key `state_dict`, strict."""
        checkpt = torch.load(os.path.join(self.cfg.model.pretrain_path), map_location="cpu", weights_only=False)
        self.model.load_state_dict(checkpt["state_dict"], strict=True)
        self.model.init()
