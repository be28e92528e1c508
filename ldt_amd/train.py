"""Score training on the HIP path: the optimizer and the host-driven training forward / backward of the eps-prediction Transformer.

Reference: trainer/Latent_SDE_Trainer.py:94-141 (`update`, `update_score`), tools/utils.py:25-101 (EMA around Adam),
model/scorenet/score.py:117-151 and model/layers.py:183-229 (what is differentiated).  Scope: the configuration the shipped YAMLs
train — LayerNorm, AdaLN, attention with 8-, 16-, 32- or 64-wide heads (the hybrid config's Score: hidden 128, 16 heads),
unconditional, label-conditioned, or conditioned on the embedded ViPC pair (pts_condition, img_condition): the even blocks then
cross-attend to the condition tokens (completion_trainer/Latent_SDE_Trainer.py:99-145; `CompletionTrainer`), and the step hands the
gradient with respect to that pair back.  ConditionNet itself is not differentiated.

`AdamEMA` keeps fp32 master parameters, gradients, both Adam moments and the EMA in five flat device buffers (one fused
`ldt_adam_ema_step` launch per step; bf16 operand panels are derived from the masters, never trained).  `ScoreTrainStep` is what is
the Score's own around train_block's block (the AdaLN form; self-attention on the fused q | k | v panel: ldt_attention_bwd / _narrow;
cross-attention to the condition tokens: ldt_attention_bwd_cross): the operand checks, the conditioning rows c and mod with their
fp32 backward, the block loop and the sum of the condition's gradient over the cross blocks.
"""
import torch

from . import ops
from ._lib import ACT_SILU, EPI_F32
from .train_block import ModRows, TrainBlock, _t, refuse_host
from .trainer import EMAWeights


class AdamEMA(EMAWeights, torch.optim.Optimizer):
    """torch.optim.Adam wrapped in the reference's EMA (tools/utils.py:25-101), stepped by one HIP kernel.

    It is an `EMAWeights` (the sampler's `state[p]['ema']` / `swap_parameters_with_ema` contract) and a `torch.optim.Optimizer`
    (`param_groups`, `state_dict()` / `load_state_dict()` in torch Adam's layout with the extra 'ema' entry, usable by
    `torch.optim.lr_scheduler`).  Nothing is allocated until the first `step()` / `zero_grad()`: a trainer built on "cpu" or used
    for sampling only holds no optimizer memory.

    At first use every parameter becomes a view of one flat fp32 buffer and gets a `.grad` view of the flat gradient;
    `state[p]` = {'step', 'exp_avg', 'exp_avg_sq', 'ema'} are views of the other flat buffers.  The EMA swap re-points `p.data`
    and `state[p]['ema']` as upstream does; `step()` finds out which flat buffer currently plays which role and re-adopts any
    tensor that was replaced from outside (`load_state_dict`, a test assigning `state[p]`)."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0., ema_decay=0.):
        params = list(params)
        EMAWeights.__init__(self, params, ema_decay)
        defaults = dict(torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        torch.optim.Optimizer.__init__(self, params, defaults)         # state = defaultdict(dict), param_groups, hooks
        self._flat = None                                              # {'a', 'b' (parameter-sized role buffers), 'g', 'm', 'v', offsets}
        self._steps = 0
        self.last_norm = None                                          # device fp32 [3]: (sum g^2, norm, clip factor) of the last step

    # ---------------------------------------------------------------- flat buffers
    def _views(self, flat):
        return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(self.params, self._flat["off"])]

    def _ensure_flat(self):
        if not self.params:
            raise ValueError("AdamEMA: no parameters")
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("AdamEMA: parameters are on %s; the HIP path has no CPU fallback" % dev)
        if self._flat is None:
            off, n = [], 0
            for p in self.params:
                if p.dtype != torch.float32 or p.device != dev:
                    raise TypeError("AdamEMA: fp32 parameters on one device only")
                off.append(n)
                n += (p.numel() + 3) // 4 * 4                           # 16-byte aligned views
            z = lambda: torch.zeros(n, dtype=torch.float32, device=dev)
            self._flat = {"off": off, "n": n, "a": z(), "b": z(), "g": z(), "m": z(), "v": z(), "scratch": None}
        F = self._flat
        ptr = lambda flat, o: flat.data_ptr() + 4 * o
        with torch.no_grad():
            # which role buffer holds the parameters right now (the EMA swap exchanges the two)?
            role = None
            for cand, other in (("a", "b"), ("b", "a")):
                if all(p.data_ptr() == ptr(F[cand], o) for p, o in zip(self.params, F["off"])):
                    role = (cand, other)
                    break
            if role is None:                                            # first use, or parameters re-pointed from outside: adopt into 'a'
                # state entries that still live in the role buffers (an EMA in 'a' after an odd number of swaps) are copied out first:
                # the adoption below overwrites 'a', and the loop after it moves them to where their role now is
                for p in self.params:
                    st = self.state[p] if p in self.state else {}
                    if "ema" in st and st["ema"].device == dev:
                        st["ema"] = st["ema"].clone()
                src = [p.data.clone() for p in self.params]             # (the new values may themselves be views of 'a' / 'b')
                for p, v, x in zip(self.params, self._views(F["a"]), src):
                    v.copy_(x)
                    p.data = v
                role = ("a", "b")
            have_ema = [("ema" in self.state[p]) if p in self.state else False for p in self.params]
            if any(have_ema) and not all(have_ema):
                raise RuntimeError("AdamEMA: some parameters carry an EMA and others do not; the fused step updates all of them together")
            for key, flat in (("ema", F[role[1]]), ("exp_avg", F["m"]), ("exp_avg_sq", F["v"])):
                for p, o, v in zip(self.params, F["off"], self._views(flat)):
                    st = self.state[p]
                    cur = st.get(key)
                    if cur is None:
                        if key != "ema":
                            v.zero_()
                            st[key] = v
                    elif cur.data_ptr() != ptr(flat, o) or cur.device != dev:
                        v.copy_(cur)
                        st[key] = v
            for p, v in zip(self.params, self._views(F["g"])):
                if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                    if p.grad is not None:
                        v.copy_(p.grad)
                    p.grad = v
            steps = {int(self.state[p]["step"]) for p in self.params if "step" in self.state[p]}
            if len(steps) > 1:
                raise RuntimeError("AdamEMA: parameters at different step counts %s" % sorted(steps))
            self._steps = steps.pop() if steps else 0
        return F, role, all(have_ema)

    def state_dict(self):
        """torch's layout (Optimizer.state_dict) with every tensor cloned: the entries are views of the flat buffers."""
        sd = torch.optim.Optimizer.state_dict(self)
        for st in sd["state"].values():
            for k, v in st.items():
                if torch.is_tensor(v):
                    st[k] = v.detach().clone()
        return sd

    @property
    def flat_grad(self):
        return self._ensure_flat()[0]["g"]

    def zero_grad(self, set_to_none=False):
        """Zero the flat gradient; the `.grad` views stay (set_to_none is accepted and ignored: the backward writes into them)."""
        self._ensure_flat()[0]["g"].zero_()

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        """clip_grad_norm_(max_norm) (None: no clipping) + Adam + EMA over every parameter, two reductions and one update launch; the clip
        factor never leaves the device."""
        if closure is not None:
            raise NotImplementedError("AdamEMA.step: closures are not used by the reference trainers")
        F, role, have_ema = self._ensure_flat()
        if len(self.param_groups) != 1:
            raise NotImplementedError("AdamEMA: one parameter group (the reference's Adam(model.parameters()))")
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
            raise NotImplementedError("AdamEMA: amsgrad / maximize / decoupled weight decay are not built")
        if F["scratch"] is None:
            from ._lib import ODE_SUMSQ_SCRATCH
            F["scratch"] = torch.empty(ODE_SUMSQ_SCRATCH, dtype=torch.float64, device=F["g"].device)
        self.last_norm = ops.sumsq(F["g"], max_norm=max_norm or 0.0, scratch=F["scratch"])
        self._steps += 1
        ema = F[role[1]] if self.apply_ema else None
        ops.adam_ema_step_(F[role[0]], F["g"], F["m"], F["v"], ema, self._steps, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                           g["weight_decay"], self.ema_decay, ema_init=not have_ema,
                           clip_factor=self.last_norm[2:] if max_norm is not None else None)
        step_t = torch.tensor(float(self._steps))                       # torch Adam's host-side fp32 step counter
        for p, v in zip(self.params, self._views(F[role[1]])):
            st = self.state[p]
            st["step"] = step_t.clone()
            if self.apply_ema and "ema" not in st:
                st["ema"] = v


def clip_factor_host(optimizer):
    """(total gradient norm, clip factor) of the last step as Python floats (synchronises; diagnostics and tests)."""
    n = optimizer.last_norm.cpu()
    return float(n[1]), float(n[2])


# ------------------------------------------------------------------------------------------------------------------------------
def refuse_untrainable(model, condition=None, world_size=1, *, allow_condition=False):
    """The configurations the training step does not cover, each refused with its reason before anything is launched.
    allow_condition: the caller trains on the embedded (pts_condition, img_condition) pair (`CompletionTrainer`); a raw condition dict —
    ConditionNet's inputs — is refused there too."""
    if not allow_condition and (condition is not None or getattr(model, "condition", False)):
        raise NotImplementedError("training with a ViPC / point condition (cross-attention blocks, ConditionNet) is not on this path: "
                                  "the backward covers self-attention blocks only")
    if isinstance(condition, dict):
        raise NotImplementedError("training on a raw ViPC / point condition dict {'img', 'pts'} is not on this path: ConditionNet's backward "
                                  "is missing.  Run model.c_net(condition) and pass the (pts_condition, img_condition) pair it returns, "
                                  "which freezes ConditionNet")
    if getattr(model, "unet", False):
        raise NotImplementedError("training the unet Score variant is not on this path (skip concatenations and conv shortcuts have no backward)")
    if not (isinstance(model.norm, str) and model.norm.lower() == "layer_norm"):
        raise NotImplementedError("training with norm=%r is not on this path: only layer_norm has a backward kernel" % (model.norm,))
    if float(getattr(model, "dropout", 0.) or 0.) > 0:
        raise NotImplementedError("training with dropout=%g is not on this path: the kernels have no dropout mask" % model.dropout)
    if world_size > 1:
        raise NotImplementedError("training on %d ranks is not on this path: the gradient all-reduce is a follow-up" % world_size)
    if model.hidden_size // model.num_heads not in (8, 16, 32, 64):
        raise NotImplementedError("training needs 8-, 16-, 32- or 64-wide attention heads (ldt_attention_bwd, ldt_attention_bwd_narrow); got %d"
                                  % (model.hidden_size // model.num_heads))


class ScoreTrainStep:
    """One forward + backward of `Score` for the denoising loss.  `forward` returns params (B, T, z) and keeps the saved activations;
    `backward(dparams)` fills every parameter's `.grad` view (the optimizer's flat gradient must be zeroed and attached first).

    With `condition=(pts_condition (B, hidden, S), img_condition (B, t_dim) or 0.)` (needs allow_condition=True) the even blocks
    cross-attend to the S condition tokens (score.py:149) and, without a label, c = TimeEmbedding(t) + img_condition (score.py:135).
    `backward` then returns, and keeps as `self.dcondition`, (d_pts_condition (B, hidden, S) fp32, d_img_condition (B, t_dim) fp32 or
    None when a label displaced the image condition or it was 0.): what ConditionNet's own backward would start from."""

    MAX_TOKENS = 512                                                   # ldt_attention_bwd_cross: 1 <= Nq, Nk <= 512

    def __init__(self, model, allow_condition=False):
        refuse_untrainable(model, allow_condition=allow_condition)
        self.m = model
        self.allow_condition = allow_condition
        self.saved = None
        self.dcondition = None

    def _panels(self, P, l, cross):
        """Block l's operands under blocks.pack_block's names: the packed q | k | v panel, or fc_q and fc_kv apart for a cross block."""
        A = {"wo": P["w_o"][l], "bo": P["b_o"][l], "wup": P["w_up"][l], "bup": P["b_up"][l], "wdn": P["w_dn"][l], "bdn": P["b_dn"][l]}
        if cross:
            A["wq"], A["bq"], A["wkv"], A["bkv"] = self.m._cross_panels(l)
        else:
            A["wqkv"], A["bqkv"] = P["w_qkv"][l], P["b_qkv"][l]
        return A

    # ---------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, x, t, label=None, condition=None):
        m = self.m
        refuse_host("ScoreTrainStep.forward", "x", x)
        B, T, z = x.shape
        D, H, nb = m.hidden_size, m.num_heads, m.num_blocks
        M, Sn = B * T, 0
        pts_cond = img_cond = None
        if condition is not None:                                      # every refusal before anything is launched or kept
            self.saved = None
            refuse_untrainable(m, condition, allow_condition=self.allow_condition)
            if not isinstance(condition, (tuple, list)) or len(condition) != 2:
                raise TypeError("ScoreTrainStep.forward: condition is the pair (pts_condition, img_condition), got %s" % type(condition).__name__)
            pts_cond, img_cond = condition
            if torch.is_tensor(pts_cond):
                if pts_cond.dim() != 3 or pts_cond.shape[0] != B or pts_cond.shape[1] != D:
                    raise ValueError("ScoreTrainStep.forward: pts_condition %s is not (B = %d, hidden = %d, S) channels-first"
                                     % (tuple(pts_cond.shape), B, D))
                Sn = pts_cond.shape[2]
                if not (1 <= T <= self.MAX_TOKENS and 1 <= Sn <= self.MAX_TOKENS):
                    raise NotImplementedError("training with %d query and %d condition tokens is not on this path: ldt_attention_bwd_cross takes "
                                              "1 <= Nq, Nk <= %d" % (T, Sn, self.MAX_TOKENS))
            else:
                pts_cond = None
            if not torch.is_tensor(img_cond) or label is not None:     # 0. (score.py:133), or displaced by the label (score.py:135)
                img_cond = None
            elif tuple(img_cond.shape) != (B, m.t_dim):
                raise ValueError("ScoreTrainStep.forward: img_condition %s is not (B = %d, t_dim = %d)" % (tuple(img_cond.shape), B, m.t_dim))
        P = m.packed()
        S = {"B": B, "T": T, "label": label, "img": img_cond is not None, "S": 0}
        # conditioning rows (fp32): c = TimeEmbedding(t) [+ LabelEmbedding(label)], mod = adaLN(SiLU(c)) for every block
        te = m.TimeEmbedding.mlp
        S["e_t"] = ops.sinusoid(t.to(x).float().contiguous(), m._frequencies())
        S["a_t"] = ops.sgemm(S["e_t"], te[0].weight, te[0].bias)                                  # pre-SiLU, kept
        c = ops.sgemm(S["a_t"], te[2].weight, te[2].bias, act_in=ACT_SILU)
        if label is not None:
            le = m.LabelEmbedding
            S["lab"] = label.to(x.device).long()
            S["e_l"] = le.label_emb.weight.detach()[S["lab"]].float().contiguous()                # row gather
            S["a_l"] = ops.sgemm(S["e_l"], le.mlp[0].weight, le.mlp[0].bias)
            c = ops.add_f32(c, ops.sgemm(S["a_l"], le.mlp[2].weight, le.mlp[2].bias, act_in=ACT_SILU))
        if img_cond is not None:
            c = ops.add_f32(c, img_cond.to(x.device, torch.float32).contiguous())
        S["c"] = c
        cond = None
        if pts_cond is not None:                                       # (B, hidden, S) channels-first -> token-major rows, bf16, once
            S["S"] = Sn
            cond = S["cond"] = ops.cast_pad_bf16(pts_cond.to(x.device, torch.float32).transpose(1, 2).contiguous().view(B * Sn, D), D)
        w_ada, b_ada = m.stacked_adaln()
        S["mod"] = ops.sgemm(c, w_ada, b_ada, act_in=ACT_SILU)                                    # [B, n_mod]
        mod, tb = ModRows(S["mod"], D, T), TrainBlock(ops)
        # token path
        S["x_in"] = x.contiguous().float().view(M, z)
        xin = ops.cast_pad_bf16(S["x_in"], ops.pad64(z))
        X = ops.gemm_bf16(xin, P["w_in"], P["b_in"], EPI_F32)
        S["blocks"] = []
        for l in range(nb):
            cross = cond is not None and l % 2 == 0                                               # score.py:149; layers.py:184-189 with y
            S["blocks"].append(tb.block_fwd(self._panels(P, l, cross), X, (B, H, T, Sn if cross else T, D // H), mod, l * 6 * D,
                                         y=cond if cross else None))
        S["xf"] = X
        S["hf"], out = tb.final_fwd(X, P["w_out"], P["b_out"], z, mod, nb * 6 * D)
        self.saved = S
        return out.view(B, T, z)

    # ---------------------------------------------------------------- backward
    @torch.no_grad()
    def backward(self, dparams):
        m, S = self.m, self.saved
        if S is None:
            raise RuntimeError("ScoreTrainStep.backward before forward")
        self.saved = None
        self.dcondition = None
        B, T, Sn = S["B"], S["T"], S.get("S", 0)
        d_cond = None                                                   # fp32 [B S, D]: the sum over the cross blocks, in the loop's order
        D, H, nb, z = m.hidden_size, m.num_heads, m.num_blocks, m.z_dim
        M = B * T
        dmod = torch.empty_like(S["mod"])
        mod, tb = ModRows(S["mod"], D, T, dmod), TrainBlock(ops)
        d2 = dparams.contiguous().view(M, z)
        dX = torch.zeros((M, D), dtype=torch.float32, device=d2.device)
        tb.final_bwd(m.ln_out.ln, d2, S["xf"], S["hf"], dX, mod, nb * 6 * D)
        for l in reversed(range(nb)):
            blk, sb = m.Transformer[l], S["blocks"][l]
            if "kv" in sb:                                                                        # cross-attention to the condition tokens
                d_cond = tb.block_bwd(blk, sb, dX, (B, H, T, Sn, D // H), ops.attention_bwd_cross, mod, l * 6 * D, y=S["cond"], dy_sum=d_cond)
            else:
                tb.block_bwd(blk, sb, dX, (B, H, T, T, D // H), None, mod, l * 6 * D)
        tb.linear_bwd(m.ln_in, dX, S["x_in"], want_dx=False)                                        # score.py:110
        # conditioning rows: fp32 linears on transposed operands
        dc = tb.adaln_bwd(dmod, m.stacked_adaln()[0], S["c"], [blk.adaLN[1] for blk in m.Transformer] + [m.ln_out.adaLN[1]])

        def mlp2_bwd(seq, a_pre, e_in):
            """seq = Linear, SiLU, Linear on e_in with the saved pre-activation a_pre: grads into .grad, -> d e_in."""
            d_s = ops.sgemm(dc, _t(seq[2].weight.detach()))
            d_a, s_a = ops.silu_bwd(a_pre, d_s, want_act=True)
            ops.sgemm(_t(dc), _t(s_a), out=seq[2].weight.grad)
            ops.colsum(dc, out=seq[2].bias.grad)
            ops.sgemm(_t(d_a), _t(e_in), out=seq[0].weight.grad)
            ops.colsum(d_a, out=seq[0].bias.grad)
            return d_a

        mlp2_bwd(m.TimeEmbedding.mlp, S["a_t"], S["e_t"])
        if S["label"] is not None:
            le = m.LabelEmbedding
            d_a = mlp2_bwd(le.mlp, S["a_l"], S["e_l"])
            d_e = ops.sgemm(d_a, _t(le.mlp[0].weight.detach()))
            le.label_emb.weight.grad.copy_(ops.embedding_grad(d_e, S["lab"], le.label_emb.weight.shape[0]))
        if Sn or S.get("img"):                                                                       # the gradient of the condition pair
            d_pts = None if d_cond is None else d_cond.view(B, Sn, D).transpose(1, 2).contiguous()   # (B, hidden, S), as ConditionNet returns it
            self.dcondition = (d_pts, dc if S.get("img") else None)
        return self.dcondition
