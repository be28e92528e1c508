"""Training the Compressor on the HIP path, in four steps (three of them around train_block's one block): here is what is
particular to each — the operand checks and refusals, the conditioning row, the level / stage loops and the order in which the stream
gradients are added — plus `_centred_keys` and the composed `w_zkv` linear's backward.

`DecoderTrainStep`, the decoder alone with the encoder frozen (Network.py:251-268 `Compressor.sample`, :80-83
`DecoderBlock.forward` with c = None; model/Compressor/layers.py:26-42, the learned prior rows): per level the affine-form block of the N
set points on the T latent tokens, K | V handed in by the composed linear on eps_j (`ldt_attention_bwd_long`; the fp32 linears on the
latent tokens: `ldt_sgemm`; the prior rows' gradient: `ldt_rows_gather_sum`).  `backward` fills the `.grad` of decoder_parameters(model)
and returns the gradient with respect to the latents (`d_eps`).

`TopDownTrainStep` (section 4.16): everything from the encoder's outputs upward (Network.py:208-233, `top_down`): per level the
posterior block `decoder[l].att` (the affine form again: the T latent tokens attend to the N points of the running set stream, level 0 to
themselves; K / V from the RAW stream, quirk Q2), the `decoder[l].prior` head, the reparameterised draw with its KL term, and the decoder
block.  Its backward is ONE interleaved pass: the posterior of level j + 1 reads the set stream o_{j+1}, so its K/V gradient has to be in
`dX` before decoder block j runs backward.  Kernels on top of the decoder step's: `ldt_attention_bwd_wide` (T queries on N keys; level 0's
T on T is `ldt_attention_bwd_cross`), `ldt_reparam_kl_bwd`, `ldt_silu_bwd`.  It returns the gradient with respect to the encoder outputs
(`d_enc_out`), where the encoder backward starts.

`EncoderTrainStep` (section 4.17): what lies between the frozen front (`Compressor.front`) and the top-down half (Network.py:200-205):
ActNorm, then per stage the AdaLN-form blocks (K / V from the RAW token stream) and the FinalLayer `conv_out`, all modulated by rows of ONE
fp32 linear on SiLU(pos).  Its backward starts from `d_enc_out`, runs the stages in reverse with the FinalLayer's gradient ADDED to the
running stream gradient (the stream runs on into the next stage), and ends in `ldt_actnorm_bwd`; it returns (d_tokens, d_pos), where the
grouper's and the position embedding's backward start.

`FrontTrainStep` (section 4.19): the front itself (Network.py:189-198) in TRAINING mode — the input conv, FPS / kNN grouping with 'anchor'
normalisation, the three PreExtraction convs with batch-statistics BatchNorm (`ldt_bn_stats`, `ldt_bn_relu_fwd`), the max over the
neighbours with its arg-max kept (`ldt_maxpool_argmax`), MiniPointnet on the centres.  Its backward starts from (d_tokens, d_pos):
`ldt_maxpool_relu_bwd`, `ldt_bn_relu_bwd`, the bf16 linears' backward of train_block, `ldt_group_normalize_bwd`, the fp32 linears through
`ldt_sgemm` on transposed operands.  The cloud is data: nothing is returned.
"""
import torch

from . import _lib, ops
from ._lib import ACT_SILU, EPI_BF16
from .layers import conv_w
from .train_block import ModRows, TrainBlock, _grad2d, _t, refuse_host

HEAD_DIM = 32                                                          # ldt_attention_bwd_long: the Compressor's 128 / 4


def decoder_parameters(model):
    """The parameters a decoder step trains, in module order (`named_parameters` order restricted to the decoder side)."""
    names = ("fc_q", "fc_kv", "fc_o", "norm1", "norm2", "mlp")
    out = []
    for name, p in model.named_parameters():
        parts = name.split(".")
        if parts[0] in ("output", "init_set"):
            out.append((name, p))
        elif parts[0] == "decoder" and (parts[2] == "ln" or (parts[2] == "att1" and parts[3] in names)):
            out.append((name, p))
    return out


def topdown_parameters(model):
    """The parameters a top-down step trains, in module order: decoder_parameters plus, per level, the posterior block `att` and the
    `prior` head."""
    names = ("fc_q", "fc_kv", "fc_o", "norm1", "norm2", "mlp")
    dec = {n for n, _ in decoder_parameters(model)}
    out = []
    for name, p in model.named_parameters():
        parts = name.split(".")
        if name in dec or (parts[0] == "decoder" and ((parts[2] == "att" and parts[3] in names) or parts[2] == "prior")):
            out.append((name, p))
    return out


# ---------------------------------------------------------------- the pieces both steps run, each written once
def _f32(t):
    return t.detach().float().contiguous()


def _decoder_level_fwd(P, X, e2, j, S, B, H, N, T, L, z):
    """Decoder block j of the top-down pass (reversed(self.decoder), Network.py:263) on the set stream X, in place -> its tape."""
    Pd = P["dec"][L - 1 - j]
    kv = ops.sgemm(e2[:, z * j: z * (j + 1)], Pd["w_zkv"], Pd["b_zkv"], out_bf16=True)                    # [B T, 2 C] = K | V, composed linear
    S["w_zkv_t"][j] = _t(Pd["w_zkv"])                                                                     # [z, 2 C]: d_eps_j = dkv W_zkv
    return TrainBlock(ops).block_fwd(Pd["att1"], X, (B, H, N, T, HEAD_DIM), kv=kv)


def _decoder_level_bwd(d, sb, dX, e_j, w_zkv_t, d_eps_j, B, H, N, T):
    """Backward of decoder block `d` = decoder[L - 1 - j]: dX becomes the gradient of the block's input, d_eps_j is written."""
    blk = d.att1
    dkv = TrainBlock(ops).block_bwd(blk, sb, dX, (B, H, N, T, HEAD_DIM), ops.attention_bwd_long)
    # kv = eps_j W_zkv^T + b_zkv with W_zkv = W_kv W_ln, b_zkv = W_kv b_ln + b_kv: the composed linear hands its gradient to both factors
    dkv32 = ops.widen_bf16(dkv)
    w_kv, w_ln, b_ln = _f32(conv_w(blk.fc_kv)), _f32(conv_w(d.ln)), _f32(d.ln.bias)
    C = dX.shape[1]
    dW_zkv = ops.sgemm(_t(dkv32), _t(e_j))                                                # [2 C, z]
    db_zkv = ops.colsum(dkv32)                                                            # [2 C]
    ops.sgemm(torch.cat([dW_zkv, db_zkv[:, None]], 1), torch.cat([w_ln, b_ln[:, None]], 1), out=_grad2d(blk.fc_kv.weight))   # dW_zkv W_ln^T + db_zkv (x) b_ln
    blk.fc_kv.bias.grad.copy_(db_zkv)
    w_kv_t = _t(w_kv)                                                                     # [C, 2 C]
    ops.sgemm(w_kv_t, _t(dW_zkv), out=_grad2d(d.ln.weight))                               # W_kv^T dW_zkv  [C, z]
    ops.sgemm(db_zkv.view(1, 2 * C), w_kv_t, out=d.ln.bias.grad.view(1, C))               # W_kv^T db_zkv
    ops.sgemm(dkv32, w_zkv_t, out=d_eps_j)                                                # dkv W_zkv


def _output_bwd(m, dset, xf, M):
    """The output conv C -> 3 (fp32 on both sides of a 3-wide linear) -> dX fp32 [M, C], the gradient of the residual stream."""
    d2 = dset.detach().float().contiguous().view(M, 3)
    ops.wgrad(d2, xf, out=_grad2d(m.output.weight))
    ops.colsum(d2, out=m.output.bias.grad)
    return ops.sgemm(d2, _t(_f32(conv_w(m.output))))


def _start(m, who, B, T, N, keep_mask):
    """The checks and the first rows both forwards share -> (keep_mask, src map of rows_gather_sum, X fp32 [B N, C])."""
    refuse_undecodable(m, N, T)
    if keep_mask is None:
        keep_mask = m._presence(B, N)
    if keep_mask is not None:
        keep_mask = keep_mask.to(torch.bool)
        if tuple(keep_mask.shape) != (B, m.max_outputs) or not bool((keep_mask.sum(1) == N).all()):
            raise ValueError("%s.forward: keep_mask must be (B = %d, max_outputs = %d) with %d kept rows per sample"
                             % (who, B, m.max_outputs, N))
    # which row of each sample every prior row became (ldt_rows_gather_sum's map), built once here where the mask is
    src = ops.prior_row_map(torch.ones((B, N), dtype=torch.bool) if keep_mask is None else keep_mask)
    return keep_mask, src


def refuse_undecodable(model, num_points=None, tokens=None):
    """The configurations the decoder step does not cover, each refused with its reason before anything is launched (works on CPU
    parameters).  num_points / tokens: the set and latent lengths of the call (default: cfg.outsize, cfg.z_scales)."""
    if getattr(model, "class_condition", False):
        raise NotImplementedError("training the decoder with class_condition is not on this path: the label's AdaLN branch of the decoder "
                                  "blocks has no backward here")
    if getattr(model, "decoder_act", None) is not None:
        raise NotImplementedError("training the decoder with decoder_act=%r is not on this path: the activation behind the norms has no "
                                  "backward kernel" % (model.decoder_act,))
    if not (isinstance(model.norm, str) and model.norm.lower() == "layer_norm"):
        raise NotImplementedError("training the decoder with norm=%r is not on this path: only layer_norm has a backward kernel" % (model.norm,))
    if model.max_outputs is None:
        raise NotImplementedError("training the decoder with max_outputs: None (the mixture InitialSet) is not on this path: only the learned "
                                  "prior rows have a backward")
    if float(getattr(model, "decoder_dropout_p", 0.) or 0.) > 0:
        raise NotImplementedError("training the decoder with decoder_dropout_p=%g is not on this path: the kernels have no dropout mask"
                                  % model.decoder_dropout_p)
    if model.hidden_dim % model.num_heads or model.hidden_dim // model.num_heads != HEAD_DIM:
        raise NotImplementedError("training the decoder needs %d-wide attention heads (ldt_attention_bwd_long); got hidden %d / %d heads"
                                  % (HEAD_DIM, model.hidden_dim, model.num_heads))
    N = model.outsize if num_points is None else int(num_points)
    T = model.z_scales if tokens is None else int(tokens)
    if not (1 <= N <= DecoderTrainStep.MAX_QUERIES and 1 <= T <= DecoderTrainStep.MAX_KEYS):
        raise NotImplementedError("training the decoder with %d set points on %d latent tokens is not on this path: ldt_attention_bwd_long takes "
                                  "1 <= Nq <= %d, 1 <= Nk <= %d" % (N, T, DecoderTrainStep.MAX_QUERIES, DecoderTrainStep.MAX_KEYS))
    if N > model.max_outputs:
        raise ValueError("%d set points from %d prior rows" % (N, model.max_outputs))


class DecoderTrainStep:
    """One forward + backward of the Compressor's decoder.  `forward(eps)` returns the decoded set (B, N, 3) and keeps the tape;
    `backward(dset)` fills the decoder-side `.grad`s (allocated here when a parameter has none; an optimizer's flat views are written in
    place) and returns d_eps (B, T, n_layers * z_dim), kept as `self.d_eps`."""

    MAX_QUERIES = _lib.ATTN_BWD_LONG_MAX_QUERIES                       # ldt_attention_bwd_long: 1 <= Nq <= 8192
    MAX_KEYS = _lib.ATTN_BWD_LONG_MAX_KEYS                             #                         1 <= Nk <= 512

    def __init__(self, model):
        refuse_undecodable(model)
        self.m = model
        self.saved = None
        self.d_eps = None

    # ---------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, eps, num_points=None, keep_mask=None):
        m = self.m
        refuse_host("DecoderTrainStep.forward", "eps", eps)
        self.saved = None
        B, T, Z = eps.shape
        L, z, C, H = m.n_layers, m.z_dim, m.hidden_dim, m.num_heads
        if Z != L * z:
            raise ValueError("DecoderTrainStep.forward: eps %s is not (B, tokens, n_layers * z_dim = %d)" % (tuple(eps.shape), L * z))
        N = m.outsize if num_points is None else int(num_points)
        keep_mask, src = _start(m, "DecoderTrainStep", B, T, N, keep_mask)
        P = m.packed()
        e2 = eps.detach().float().contiguous().view(B * T, Z)
        S = {"B": B, "N": N, "T": T, "eps": e2, "src": src.to(eps.device), "w_zkv_t": [None] * L, "levels": []}
        X = m._initial_set(P, B, N, keep_mask).clone()                  # fp32 [B N, C]: the residual stream, updated in place below
        for j in range(L):
            S["levels"].append(_decoder_level_fwd(P, X, e2, j, S, B, H, N, T, L, z))
        S["xf"] = X
        out = ops.sgemm(X, P["w_out"], P["b_out"])                      # Conv1d C -> 3, Network.py:266
        self.saved = S
        return out.view(B, N, 3)

    # ---------------------------------------------------------------- backward
    @torch.no_grad()
    def backward(self, dset):
        m, S = self.m, self.saved
        if S is None:
            raise RuntimeError("DecoderTrainStep.backward before forward")
        self.saved = None
        self.d_eps = None
        B, N, T = S["B"], S["N"], S["T"]
        L, z, C, H = m.n_layers, m.z_dim, m.hidden_dim, m.num_heads
        M = B * N
        if tuple(dset.shape) != (B, N, 3):
            raise ValueError("DecoderTrainStep.backward: dset %s is not (%d, %d, 3)" % (tuple(dset.shape), B, N))
        for _, p in decoder_parameters(m):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        dX = _output_bwd(m, dset, S["xf"], M)
        d_eps = torch.empty((B * T, L * z), dtype=torch.float32, device=dX.device)
        for j in reversed(range(L)):
            _decoder_level_bwd(m.decoder[L - 1 - j], S["levels"][j], dX, S["eps"][:, z * j: z * (j + 1)], S["w_zkv_t"][j],
                               d_eps[:, z * j: z * (j + 1)], B, H, N, T)
        # the learned prior rows: every sample started from them (all, or its kept ones packed to the front)
        m.init_set.prior.grad.copy_(ops.rows_gather_sum(dX, S["src"], N))
        self.d_eps = d_eps.view(B, T, L * z)
        return self.d_eps


def _centred_keys(A, y, kv, B, nk):
    """K | V of a posterior block for its backward, with each sample's mean key taken off K: bf16(y W_k^T + b_k - mean_j K_j), formed from
    the fp32 accumulators by the forward's GEMM with a per-sample bias.  Neither P (softmax is invariant under a logit shift common to a
    row) nor dQ = scale sum_j dS_j k_j (sum_j dS_j = 0) depends on a common shift of the keys, and dK, dV do not read the key values
    beyond P.  What does depend on it is the error: the kernel takes D = rowsum(dO o O) from the saved bf16 O, and the error of D enters
    dQ times the P-weighted MEAN key.  The points of the set stream share a large common component (they all start from prior rows that
    the same blocks moved), so that term dominated dQ's error (rel-MSE 1.1e-4 of dQ at the tiny fixture's last
    level, 8.5e-6 with the mean taken off)."""
    C = A["C"]
    sums = torch.stack([ops.colsum(kv[b * nk:(b + 1) * nk, :C]) for b in range(B)])                       # [B, C] fp32, fixed order
    off = torch.eye(C, dtype=torch.float32, device=kv.device) * (-1.0 / nk)
    bias = ops.sgemm(sums, off, A["bkv"][:C].contiguous())                                                # b_k - mean key, per sample
    kvc = kv.clone()
    for b in range(B):
        ops.gemm_bf16(y[b * nk:(b + 1) * nk], A["wkv"][:C], bias[b], EPI_BF16, out=kvc[b * nk:(b + 1) * nk, :C])
    return kvc


def refuse_untrainable_topdown(model, num_points=None, tokens=None):
    """What the top-down step does not cover: the posterior's attention limits first (T queries on N keys: ldt_attention_bwd_wide; level
    0's T on T: ldt_attention_bwd_cross), then everything refuse_undecodable refuses.  Works on CPU parameters."""
    N = model.outsize if num_points is None else int(num_points)
    T = model.z_scales if tokens is None else int(tokens)
    if not (1 <= T <= TopDownTrainStep.MAX_TOKENS and 1 <= N <= TopDownTrainStep.MAX_POINTS):
        raise NotImplementedError("training the top-down half with %d latent tokens on %d set points is not on this path: the posterior's "
                                  "ldt_attention_bwd_wide takes 1 <= Nq <= %d, 1 <= Nk <= %d"
                                  % (T, N, TopDownTrainStep.MAX_TOKENS, TopDownTrainStep.MAX_POINTS))
    refuse_undecodable(model, num_points, tokens)


class TopDownTrainStep:
    """One forward + backward of the Compressor's top-down half (Network.py:208-233).  `forward(enc_out, post_noise)` returns the decoded
    set (B, N, 3), all_eps (B, T, n_layers * z_dim) and kl_sample_sum (B, n_layers), and keeps the tape; `backward(dset, kl_scale)` fills
    every `.grad` of topdown_parameters(model) for  loss = <dset, set> + kl_scale * sum(kl)  and returns d_enc_out, a list of n_layers
    fp32 (B, T, C) tensors (index i: the gradient of enc_out[i]), kept as `self.d_enc_out`."""

    MAX_TOKENS = _lib.ATTN_BWD_WIDE_MAX_QUERIES                        # ldt_attention_bwd_wide: 1 <= Nq <= 512 (and ldt_attention_bwd_cross at level 0)
    MAX_POINTS = _lib.ATTN_BWD_WIDE_MAX_KEYS                           #                         1 <= Nk <= 8192

    def __init__(self, model):
        refuse_untrainable_topdown(model)
        self.m = model
        self.saved = None
        self.d_eps = None
        self.d_enc_out = None

    # ---------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, enc_out, post_noise, num_points=None, keep_mask=None):
        m = self.m
        L, z, C, H = m.n_layers, m.z_dim, m.hidden_dim, m.num_heads
        enc_out, post_noise = list(enc_out), list(post_noise)
        refuse_host("TopDownTrainStep.forward", "an operand", *enc_out, *post_noise)
        self.saved = None
        if len(enc_out) != L or len(post_noise) != L:
            raise ValueError("TopDownTrainStep.forward: %d encoder outputs and %d posterior draws for %d levels" % (len(enc_out), len(post_noise), L))
        B, T = enc_out[0].shape[0], enc_out[0].shape[1]
        for t in enc_out:
            if tuple(t.shape) != (B, T, C):
                raise ValueError("TopDownTrainStep.forward: encoder output %s is not (B = %d, tokens = %d, hidden = %d)" % (tuple(t.shape), B, T, C))
        for t in post_noise:
            if tuple(t.shape) != (B, T, z):
                raise ValueError("TopDownTrainStep.forward: posterior draw %s is not (B = %d, tokens = %d, z_dim = %d)" % (tuple(t.shape), B, T, z))
        N = m.outsize if num_points is None else int(num_points)
        refuse_untrainable_topdown(m, N, T)
        keep_mask, src = _start(m, "TopDownTrainStep", B, T, N, keep_mask)
        P = m.packed()
        dev = enc_out[0].device
        all_eps = torch.empty((B * T, L * z), dtype=torch.float32, device=dev)
        tb = TrainBlock(ops)
        S = {"B": B, "N": N, "T": T, "eps": all_eps, "src": src.to(dev), "w_zkv_t": [None] * L, "levels": [], "post": []}
        X = m._initial_set(P, B, N, keep_mask).clone()                  # fp32 [B N, C]: the set stream o, updated in place below
        kl_sums = []
        for j in range(L):
            Pd = P["dec"][L - 1 - j]
            A = Pd["att"]
            xj = enc_out[-j - 1].detach().float().contiguous().view(B * T, C).clone()                     # the token stream of this level, updated in place
            # compute_posterior(x, o) (Network.py:61-78): att(x, o) with K / V from the RAW set stream (quirk Q2); level 0: att(x, x)
            y, nk = (ops.cast_pad_bf16(xj, ops.pad64(C)), T) if j == 0 else (ops.cast_pad_bf16(X, ops.pad64(C)), N)
            pb = tb.block_fwd(A, xj, (B, H, T, nk, HEAD_DIM), kv=ops.gemm_bf16(y, A["wkv"], A["bkv"], EPI_BF16))
            pb["y"], pb["x3"] = y, xj
            pb["kv"] = _centred_keys(A, y, pb["kv"], B, nk)                                               # the backward's K | V (the forward is done with its own)
            pb["post"] = ops.sgemm(xj, Pd["w_prior"], Pd["b_prior"], act_in=ACT_SILU)                     # SiLU -> Conv1d C -> 2 z
            pb["noise"] = post_noise[j].detach().to(dev, torch.float32).contiguous().view(B * T, z)
            kl_sums.append(ops.reparam_kl(pb["post"], pb["noise"], all_eps[:, z * j: z * (j + 1)], m.min_sigma, 10., T)[4])
            S["post"].append(pb)
            S["levels"].append(_decoder_level_fwd(P, X, all_eps, j, S, B, H, N, T, L, z))
        S["xf"] = X
        out = ops.sgemm(X, P["w_out"], P["b_out"])                      # Conv1d C -> 3, Network.py:233
        self.saved = S
        return out.view(B, N, 3), all_eps.view(B, T, L * z), torch.stack(kl_sums, 1)

    # ---------------------------------------------------------------- backward
    @torch.no_grad()
    def backward(self, dset, kl_scale):
        m, S = self.m, self.saved
        if S is None:
            raise RuntimeError("TopDownTrainStep.backward before forward")
        self.saved = None
        self.d_enc_out = None
        B, N, T = S["B"], S["N"], S["T"]
        L, z, C, H = m.n_layers, m.z_dim, m.hidden_dim, m.num_heads
        M = B * N
        if tuple(dset.shape) != (B, N, 3):
            raise ValueError("TopDownTrainStep.backward: dset %s is not (%d, %d, 3)" % (tuple(dset.shape), B, N))
        for _, p in topdown_parameters(m):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        dX = _output_bwd(m, dset, S["xf"], M)                           # the complete gradient of o_L
        tb = TrainBlock(ops)
        d_eps = torch.empty((B * T, L * z), dtype=torch.float32, device=dX.device)
        d_enc = [None] * L
        for j in reversed(range(L)):                                    # dX: the complete gradient of o_{j+1}
            d, pb = m.decoder[L - 1 - j], S["post"][j]
            dej = d_eps[:, z * j: z * (j + 1)]
            _decoder_level_bwd(d, S["levels"][j], dX, S["eps"][:, z * j: z * (j + 1)], S["w_zkv_t"][j], dej, B, H, N, T)
            # eps_j = mu + exp(clamp(logvar) / 2) noise and kl_scale * kl (Network.py:26-29, 219-224)
            dpost = ops.reparam_kl_bwd(pb["post"], pb["noise"], dej, kl_scale, m.min_sigma, 10.)
            # (mu | logvar) = prior.1(SiLU(x3)), fp32 (Network.py:76)
            lin = d.prior[1]
            dact = ops.sgemm(dpost, _t(_f32(conv_w(lin))))
            dXp, act = ops.silu_bwd(pb["x3"], dact, want_act=True)       # the gradient of the token stream behind the posterior block
            ops.wgrad(dpost, act, out=_grad2d(lin.weight))
            ops.colsum(dpost, out=lin.bias.grad)
            nk = T if j == 0 else N
            dkv = tb.block_bwd(d.att, pb, dXp, (B, H, T, nk, HEAD_DIM), ops.attention_bwd_cross if j == 0 else ops.attention_bwd_wide)
            dy = tb.linear_bwd(d.att.fc_kv, dkv, pb["y"])                   # [B nk, C] fp32: into the K / V source
            if j == 0:
                ops.add_f32(dXp, dy, out=dXp)                           # att(x, x): the block attends to its own input
            else:
                ops.add_f32(dX, dy, out=dX)                             # att(x, o_j): ADDED to the set stream's gradient before decoder block j - 1 runs
            d_enc[L - 1 - j] = dXp.view(B, T, C)
        m.init_set.prior.grad.copy_(ops.rows_gather_sum(dX, S["src"], N))
        self.d_eps = d_eps.view(B, T, L * z)
        self.d_enc_out = d_enc
        return d_enc


# ---------------------------------------------------------------- the encoder: ActNorm and the AdaLN stages
def encoder_parameters(model):
    """The parameters an encoder step trains, in module order: conv_in's ActNorm, and per stage the AdaLN blocks and the FinalLayer
    (`norm1` / `norm2` / `norm` have no parameters under AdaLN)."""
    names = ("fc_q", "fc_kv", "fc_o", "adaLN", "mlp")
    out = []
    for name, p in model.named_parameters():
        parts = name.split(".")
        if parts[0] == "conv_in" and parts[1] in ("shift", "log_scale"):
            out.append((name, p))
        elif parts[0] == "encoder" and ((parts[2] == "atts" and parts[4] in names) or (parts[2] == "conv_out" and parts[3] in ("adaLN", "ln"))):
            out.append((name, p))
    return out


def refuse_untrainable_encoder(model, tokens=None):
    """The configurations the encoder step does not cover, each refused with its reason before anything is launched (works on CPU
    parameters).  tokens: the token count of the call (default: cfg.z_scales).  `ActNorm: ~` is covered: the step then has no ActNorm."""
    from .layers import MLP
    if isinstance(model.pos_embedding, MLP):
        raise NotImplementedError("training the encoder with pos_embedding: mlp is not on this path: a per-token position condition modulates "
                                  "every token with its own row, and the modulation backward sums over a sample's tokens")
    if getattr(model, "class_condition", False):
        raise NotImplementedError("training the encoder with class_condition is not on this path: the label embedding added to the position "
                                  "condition has no backward here")
    if model.AdaLN is not None and not model.AdaLN:
        raise NotImplementedError("training the encoder with AdaLN: False is not on this path: the backward covers the AdaLN blocks only")
    if not (isinstance(model.norm, str) and model.norm.lower() == "layer_norm"):
        raise NotImplementedError("training the encoder with norm=%r is not on this path: only layer_norm has a backward kernel" % (model.norm,))
    if float(getattr(model, "encoder_dropout_p", 0.) or 0.) > 0:
        raise NotImplementedError("training the encoder with encoder_dropout_p=%g is not on this path: the kernels have no dropout mask"
                                  % model.encoder_dropout_p)
    if model.hidden_dim % model.num_heads or model.hidden_dim // model.num_heads != HEAD_DIM:
        raise NotImplementedError("training the encoder needs %d-wide attention heads (ldt_attention_bwd_cross as the decoder's kernels take "
                                  "them); got hidden %d / %d heads" % (HEAD_DIM, model.hidden_dim, model.num_heads))
    T = model.z_scales if tokens is None else int(tokens)
    if not 1 <= T <= EncoderTrainStep.MAX_TOKENS:
        raise NotImplementedError("training the encoder with %d tokens is not on this path: ldt_attention_bwd_cross takes 1 <= Nq, Nk <= %d"
                                  % (T, EncoderTrainStep.MAX_TOKENS))


class EncoderTrainStep:
    """One forward + backward of the Compressor's encoder (Network.py:200-205: ActNorm, then per stage `encoder_layers` AdaLN blocks that
    attend to their own RAW input (layers.py:210-219 with y = x, quirk Q2) and the FinalLayer `conv_out`, :41-45).  `forward(tokens, pos)`
    takes the grouped tokens (B, T, hidden) BEFORE ActNorm and the position condition (B, p_dim) (`Compressor.front`) and returns the
    n_layers stage outputs, fresh fp32 (B, T, hidden) tensors, keeping the tape; `backward(d_enc_out)` fills every `.grad` of
    encoder_parameters(model) and returns (d_tokens (B, T, hidden), d_pos (B, p_dim)), kept as `self.d_tokens` / `self.d_pos`: where the
    grouper's and the position embedding's backward would start."""

    MAX_TOKENS = 512                                                   # ldt_attention_bwd_cross: 1 <= Nq, Nk <= 512

    def __init__(self, model):
        refuse_untrainable_encoder(model)
        self.m = model
        self.saved = None
        self.d_tokens = None
        self.d_pos = None

    def _adaln(self):
        """Every block's and FinalLayer's adaLN.1 in the order the modulation row is laid out: per stage the blocks (6 C each: shift_msa,
        scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp), then conv_out (2 C: shift, scale)."""
        return [lin for e in self.m.encoder for lin in [a.adaLN[1] for a in e.atts] + [e.conv_out.adaLN[1]]]

    # ---------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, tokens, pos):
        m = self.m
        refuse_host("EncoderTrainStep.forward", "an operand", tokens, pos)
        self.saved = None
        C, H = m.hidden_dim, m.num_heads
        if tokens.dim() != 3 or tokens.shape[2] != C:
            raise ValueError("EncoderTrainStep.forward: tokens %s is not (B, tokens, hidden = %d)" % (tuple(tokens.shape), C))
        B, T = tokens.shape[0], tokens.shape[1]
        if tuple(pos.shape) != (B, m.p_dim):
            raise ValueError("EncoderTrainStep.forward: pos %s is not (B = %d, p_dim = %d)" % (tuple(pos.shape), B, m.p_dim))
        refuse_untrainable_encoder(m, T)
        M = B * T
        P = m.packed()
        S = {"B": B, "T": T, "stages": []}
        X = tokens.detach().float().contiguous().view(M, C).clone()     # the token stream x, updated in place below
        if m.ActNorm is not None:
            if P["an_shift"].numel() not in (C, T * C):
                raise ValueError("EncoderTrainStep.forward: ActNorm holds %d values for %d tokens of %d channels" % (P["an_shift"].numel(), T, C))
            ops.actnorm_(X, P["an_shift"], P["an_logs"], M * C // P["an_shift"].numel())                  # Network.py:200-201
        S["pos"] = pos.detach().float().contiguous()
        lins = self._adaln()
        S["w_ada"] = torch.cat([_f32(l.weight) for l in lins], 0)
        S["mod"] = ops.sgemm(S["pos"], S["w_ada"], torch.cat([_f32(l.bias) for l in lins], 0), act_in=ACT_SILU)   # [B, n_mod]
        mod, tb = ModRows(S["mod"], C, T), TrainBlock(ops)
        # the backward's K | V: the raw tokens share a large common component (mean key / rms key 0.8 - 0.9 at the tiny fixture), the case
        # _centred_keys was written for (section 4.17: dQ rel-MSE 1e-4 - 2e-4 from D = rowsum(dO o O) of the bf16 O, 1e-7 - 4e-7 centred)
        centred = lambda A: lambda y, kv: _centred_keys(A, y, kv, B, T)
        outs, m0 = [], 0
        for Pe in P["enc"]:
            st = {"blocks": []}
            for A in Pe["atts"]:                                        # K / V from the RAW x (Network.py:44, quirk Q2); the first x1 is ActNorm's output z
                st["blocks"].append(tb.block_fwd(A, X, (B, H, T, T, HEAD_DIM), mod, m0, y=X, kv_bwd=centred(A)))
                m0 += 6 * C
            # conv_out, a FinalLayer (layers.py:240-246): the stream x itself runs on into the next stage
            st["xf"] = X.clone()
            st["hf"], out = tb.final_fwd(X, Pe["out"]["w"], Pe["out"]["b"], Pe["out"]["n_out"], mod, m0)
            outs.append(out.view(B, T, -1))
            m0 += 2 * C
            S["stages"].append(st)
        self.saved = S
        return outs

    # ---------------------------------------------------------------- backward
    @torch.no_grad()
    def backward(self, d_enc_out):
        m, S = self.m, self.saved
        if S is None:
            raise RuntimeError("EncoderTrainStep.backward before forward")
        self.saved = None
        self.d_tokens = self.d_pos = None
        B, T = S["B"], S["T"]
        C, H, L, E = m.hidden_dim, m.num_heads, m.n_layers, m.encoder_layers
        M = B * T
        d_enc_out = list(d_enc_out)
        if len(d_enc_out) != L or any(not torch.is_tensor(t) or tuple(t.shape) != (B, T, C) for t in d_enc_out):
            raise ValueError("EncoderTrainStep.backward: d_enc_out is not %d tensors (%d, %d, %d)" % (L, B, T, C))
        if any(not t.is_cuda for t in d_enc_out):
            raise RuntimeError("EncoderTrainStep.backward: a gradient is on the CPU; the HIP path has no CPU fallback")
        for _, p in encoder_parameters(m):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        dmod = torch.empty_like(S["mod"])
        mod, tb = ModRows(S["mod"], C, T, dmod), TrainBlock(ops)
        dX = torch.zeros((M, C), dtype=torch.float32, device=dmod.device)    # the gradient of the stream x: every later stage's is already in it
        for i in reversed(range(L)):
            enc, st, m0 = m.encoder[i], S["stages"][i], i * (6 * E + 2) * C
            # enc_out[i] = conv_out.ln(mod(LN(x)))                                                  (layers.py:240-246): ADDED to dX
            tb.final_bwd(enc.conv_out.ln, d_enc_out[i].detach().float().contiguous().view(M, C), st["xf"], st["hf"], dX, mod, m0 + 6 * E * C)
            for k in reversed(range(E)):
                sb = st["blocks"][k]
                dy = tb.block_bwd(enc.atts[k], sb, dX, (B, H, T, T, HEAD_DIM), ops.attention_bwd_cross, mod, m0 + 6 * k * C, y=sb["y"])
                ops.add_f32(dX, dy, out=dX)                                                          # [M, C] fp32: into the raw x1
        d_pos = tb.adaln_bwd(dmod, S["w_ada"], S["pos"], self._adaln())                                 # the conditioning row
        if m.ActNorm is not None:                                                                    # z = (x - shift) exp(-log_scale), layers.py:103-107
            ci = m.conv_in
            z = S["stages"][0]["blocks"][0]["x1"] if E else S["stages"][0]["xf"]
            ops.actnorm_bwd(dX, z, _f32(ci.log_scale).view(-1), M * C // ci.shift.numel(), dx=dX, dshift=ci.shift.grad.view(-1),
                            dlog_scale=ci.log_scale.grad.view(-1))
        self.d_tokens, self.d_pos = dX.view(B, T, C), d_pos
        return self.d_tokens, self.d_pos


# ---------------------------------------------------------------- the front: input conv, grouper, position embedding
def front_parameters(model):
    """The parameters a front step trains, in module order: the input conv, the LocalGrouper (affine vectors, the three PreExtraction convs
    and their two BatchNorms) and the MiniPointnet position embedding."""
    return [(name, p) for name, p in model.named_parameters() if name.split(".")[0] in ("input", "group", "pos_embedding")]


def refuse_untrainable_front(model, num_points=None):
    """The configurations the front step does not cover, each refused with its reason before anything is launched.  num_points: the cloud
    size of the call (default: cfg.outsize)."""
    from .layers import MLP
    if model.pre_group:
        raise NotImplementedError("training the front with pre_group: True is not on this path: the gradient of the second grouper's points "
                                  "would have to run through the first grouper's neighbour max (two chained groupers)")
    if isinstance(model.pos_embedding, MLP):
        raise NotImplementedError("training the front with pos_embedding: mlp is not on this path: only the MiniPointnet position embedding "
                                  "has a backward (and the encoder step refuses a per-token position condition)")
    if getattr(model, "class_condition", False):
        raise NotImplementedError("training the front with class_condition is not on this path: the label embedding added to the position "
                                  "condition has no backward here")
    if model.group.normalize != "anchor":
        raise NotImplementedError("training the front with cluster_norm=%r is not on this path: ldt_group_normalize_bwd covers 'anchor' only"
                                  % (model.group.normalize,))
    N = model.outsize if num_points is None else int(num_points)
    T = model.z_scales
    k = N // T * 2
    if not 1 <= k <= N:
        raise NotImplementedError("training the front with %d points in %d groups is not on this path: k = N // T * 2 = %d neighbours of %d points"
                                  % (N, T, k, N))
    if model.input.weight.device.type != "cuda":
        raise RuntimeError("training the front: the parameters are on %s; the HIP path has no CPU fallback" % model.input.weight.device)


def _vec(t):
    """A small parameter vector as a fresh fp32 tensor (an optimizer's flat views are only 4-byte aligned: the kernels' 16-byte form wants more)."""
    return t.detach().float().reshape(-1).clone()


class FrontTrainStep:
    """One forward + backward of the Compressor's front (Network.py:189-198) in TRAINING mode: every BatchNorm normalises with the batch
    statistics and updates its running buffers (momentum, unbiased variance, num_batches_tracked), whatever `model.training` says.
    `forward(x)` takes the clouds (B, N, 3) and returns (tokens (B, T, hidden) BEFORE ActNorm, pos (B, p_dim)) — EncoderTrainStep.forward's
    operands — keeping the tape, the arg-max of the neighbour max and of MiniPointnet's max included; `fps_idx`, `knn_idx` and `centers`
    stay as attributes.  `backward(d_tokens, d_pos)` fills every `.grad` of front_parameters(model); the cloud is data and gets no gradient.
    The chain is unfused (ldt_grouper_mlp and the eval-folded panels are the evaluation path's): ldt_group_normalize, per BatchNorm layer a GEMM
    with fp32 output, ldt_bn_stats and ldt_bn_relu_fwd, the residual GEMM in fp32, ldt_maxpool_argmax with the ReLU on the maximum."""

    def __init__(self, model):
        refuse_untrainable_front(model)
        self.m = model
        self.saved = None
        self.fps_idx = self.knn_idx = self.centers = None

    def _bn(self, bn, z):
        """Batch statistics of z with the running buffers of `bn` updated as nn.BatchNorm1d does in training -> stats fp32 [2, C]."""
        if bn.momentum is None or not bn.track_running_stats:
            raise NotImplementedError("FrontTrainStep: a BatchNorm with momentum None or without running statistics is not on this path")
        st = ops.bn_stats(z, bn.eps, bn.running_mean, bn.running_var, bn.momentum)
        bn.num_batches_tracked += 1
        return st

    # ---------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, x):
        from ._lib import EPI_F32, EPI_RESID_F32
        from .compressor import _bf16_panel
        m = self.m
        refuse_host("FrontTrainStep.forward", "the cloud", x)
        self.saved = None
        if x.dim() != 3 or x.shape[2] != 3:
            raise ValueError("FrontTrainStep.forward: x %s is not (B, N, 3)" % (tuple(x.shape),))
        B, N, _ = x.shape
        refuse_untrainable_front(m, N)
        T, D = m.z_scales, m.hidden_dim
        k = N // T * 2
        if B * T < 2:
            raise ValueError("FrontTrainStep.forward: training-mode BatchNorm needs more than one centre per batch (B = %d, tokens = %d)" % (B, T))
        pts = x.detach().float().contiguous()
        if m.norm_input:
            pts = ops.norm_points(pts)                                  # a transform of data: no parameters
        S = {"B": B, "N": N, "T": T, "k": k, "pts": pts}
        S["feat"] = feat = ops.sgemm(pts.view(B * N, 3), _f32(conv_w(m.input)), _f32(m.input.bias)).view(B, N, D)     # Conv1d 3 -> D (:192)
        self.fps_idx = fps_idx = ops.fps(pts, T)
        self.centers = centers = ops.gather_rows(pts, fps_idx)
        self.knn_idx = knn_idx = ops.knn(pts, centers, k)
        g = m.group
        ex = g.extraction
        c1, bn1 = ex.transfer.net[0], ex.transfer.net[1]
        c2, bn2 = ex.operation[0].net1[0], ex.operation[0].net1[1]
        c3 = ex.operation[0].net2[0]
        S["alpha"] = _vec(g.affine_alpha)
        S["U"] = U = ops.group_normalize(feat, pts, fps_idx, knn_idx, S["alpha"], _vec(g.affine_beta), normalize="anchor")
        # transfer: Conv -> BatchNorm (batch statistics) -> ReLU
        S["w1"] = _bf16_panel(_f32(conv_w(c1)))                          # bf16 [D, pad64(2 D + 3)], kept for dU
        S["z1"] = z1 = ops.gemm_bf16(U, S["w1"], _f32(c1.bias), EPI_F32)
        S["st1"], S["g1"], S["b1"] = self._bn(bn1, z1), _vec(bn1.weight), _vec(bn1.bias)
        S["h1"] = h1 = ops.bn_relu_fwd(z1, S["st1"], S["g1"], S["b1"])
        # net1: Conv -> BatchNorm -> ReLU; net2: Conv, + the block's input, ReLU
        S["z2"] = z2 = ops.gemm_bf16(h1, _bf16_panel(_f32(conv_w(c2))), _f32(c2.bias), EPI_F32)
        S["st2"], S["g2"], S["b2"] = self._bn(bn2, z2), _vec(bn2.weight), _vec(bn2.bias)
        S["r"] = r = ops.bn_relu_fwd(z2, S["st2"], S["g2"], S["b2"])
        # only the GEMM operands are bf16: the residual takes h1 in fp32 and the sum stays fp32 up to the max, so that the tokens carry
        # the operand roundings alone (the evaluation path's EPI_RELU_BF16 rounds the skip and the sum as well)
        z3 = ops.bn_relu_fwd(z1, S["st1"], S["g1"], S["b1"], out_bf16=False)
        ops.gemm_bf16(r, _bf16_panel(_f32(conv_w(c3))), _f32(c3.bias), EPI_RESID_F32, out=z3, resid=z3)                # z3 = net2(r) + h1
        S["tok"], S["arg"] = ops.maxpool_argmax(z3, B * T, k, relu=True)  # max_j ReLU(z3_j) over the k neighbours (:186) = ReLU(max_j z3_j)
        # MiniPointnet on the centres (Network.py:86-101), fp32
        pe = m.pos_embedding
        S["ctr"] = ctr = centers.view(B * T, 3)
        S["y1"] = y1 = ops.sgemm(ctr, _f32(conv_w(pe.conv1)), _f32(pe.conv1.bias))
        S["sp1"], S["gp1"], S["bp1"] = self._bn(pe.bn1, y1), _vec(pe.bn1.weight), _vec(pe.bn1.bias)
        S["a1"] = a1 = ops.bn_relu_fwd(y1, S["sp1"], S["gp1"], S["bp1"], out_bf16=False)
        S["y2"] = y2 = ops.sgemm(a1, _f32(conv_w(pe.conv2)), _f32(pe.conv2.bias))
        S["sp2"], S["gp2"], S["bp2"] = self._bn(pe.bn2, y2), _vec(pe.bn2.weight), _vec(pe.bn2.bias)
        a2 = ops.bn_relu_fwd(y2, S["sp2"], S["gp2"], S["bp2"], out_bf16=False)
        S["pool"], S["argp"] = ops.maxpool_argmax(a2, B, T)              # the max over the tokens (:97)
        pos = ops.sgemm(S["pool"], _f32(pe.fc.weight), _f32(pe.fc.bias))
        m.invalidate_packed()                                            # the evaluation path folds the running buffers written above
        self.saved = S
        return S["tok"].view(B, T, D), pos

    # ---------------------------------------------------------------- backward
    def _fp32_linear_bwd(self, layer, dy, x_in, want_dx=True):
        """An fp32 linear through ldt_sgemm on transposed operands (as TrainBlock.adaln_bwd): dW, db into the .grad views -> dX = dy W."""
        ops.sgemm(_t(dy), _t(x_in), out=_grad2d(layer.weight))
        ops.colsum(dy, out=layer.bias.grad)
        return ops.sgemm(dy, _t(_f32(conv_w(layer)))) if want_dx else None

    @torch.no_grad()
    def backward(self, d_tokens, d_pos):
        m, S = self.m, self.saved
        if S is None:
            raise RuntimeError("FrontTrainStep.backward before forward")
        self.saved = None
        B, N, T, k = S["B"], S["N"], S["T"], S["k"]
        D = m.hidden_dim
        if not torch.is_tensor(d_tokens) or tuple(d_tokens.shape) != (B, T, D) or not torch.is_tensor(d_pos) or tuple(d_pos.shape) != (B, m.p_dim):
            raise ValueError("FrontTrainStep.backward: d_tokens / d_pos are not (%d, %d, %d) / (%d, %d)" % (B, T, D, B, m.p_dim))
        refuse_host("FrontTrainStep.backward", "a gradient", d_tokens, d_pos)
        for _, p in front_parameters(m):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        tb = TrainBlock(ops)
        g = m.group
        ex = g.extraction
        c1, bn1 = ex.transfer.net[0], ex.transfer.net[1]
        c2, bn2 = ex.operation[0].net1[0], ex.operation[0].net1[1]
        c3 = ex.operation[0].net2[0]
        # tok = max_j ReLU(net2(r) + h1): the gradient goes to the kept neighbour, where the token is positive
        dz3 = ops.maxpool_relu_bwd(d_tokens.detach().float().contiguous().view(B * T, D), S["tok"], S["arg"], k)          # [M, D] fp32
        dr = tb.linear_bwd(c3, dz3, S["r"][:, :D])
        ops.bn_relu_bwd(dr, S["z2"], S["st2"], S["g2"], S["b2"], dx=dr, dgamma=bn2.weight.grad, dbeta=bn2.bias.grad)      # dr becomes dz2
        dh1 = tb.linear_bwd(c2, dr, S["h1"][:, :D])
        ops.add_f32(dh1, dz3, out=dh1)                                   # the residual: net2's input h1 is also added to its output
        ops.bn_relu_bwd(dh1, S["z1"], S["st1"], S["g1"], S["b1"], dx=dh1, dgamma=bn1.weight.grad, dbeta=bn1.bias.grad)    # dh1 becomes dz1
        # the transfer conv at the padded width of U (2 D + 3 columns are no 16-byte row for a GEMM's output): dW's padding columns are
        # dropped, dU's are zero (the panel's padding rows) and ldt_group_normalize_bwd reads the first 2 D + 3 only
        _grad2d(c1.weight).copy_(ops.wgrad(dh1, S["U"])[:, :2 * D + 3])
        ops.colsum(dh1, out=c1.bias.grad)
        dU = ops.dgrad(ops.cast_pad_bf16(dh1, ops.pad64(D)), ops.transpose_cast_bf16(S["w1"]))       # [M, pad64(2 D + 3)] fp32
        dalpha, dbeta, dfeat = ops.group_normalize_bwd(dU, S["feat"], S["pts"], self.fps_idx, self.knn_idx, S["alpha"])
        g.affine_alpha.grad.view(-1).copy_(dalpha)
        g.affine_beta.grad.view(-1).copy_(dbeta)
        self._fp32_linear_bwd(m.input, dfeat.view(B * N, D), S["pts"].view(B * N, 3), want_dx=False)                      # the cloud is data
        # MiniPointnet
        pe = m.pos_embedding
        dpool = self._fp32_linear_bwd(pe.fc, d_pos.detach().float().contiguous(), S["pool"])
        da2 = ops.maxpool_relu_bwd(dpool, S["pool"], S["argp"], T)
        ops.bn_relu_bwd(da2, S["y2"], S["sp2"], S["gp2"], S["bp2"], dx=da2, dgamma=pe.bn2.weight.grad, dbeta=pe.bn2.bias.grad)
        da1 = self._fp32_linear_bwd(pe.conv2, da2, S["a1"])
        ops.bn_relu_bwd(da1, S["y1"], S["sp1"], S["gp1"], S["bp1"], dx=da1, dgamma=pe.bn1.weight.grad, dbeta=pe.bn1.bias.grad)
        self._fp32_linear_bwd(pe.conv1, da1, S["ctr"], want_dx=False)     # the centres are data
