"""Training the Compressor's decoder on the HIP path: the host-driven top-down forward that keeps what the backward needs, and the backward
from the gradient of the decoded set down to the decoder-side parameters and the latents.

Reference: model/Compressor/Network.py:251-268 (`Compressor.sample`, what is differentiated), :80-83 (`DecoderBlock.forward` with c = None),
model/layers.py:183-200, 224-226 (the no-condition ResidualBlock: affine LayerNorm, attention of the set on the latent tokens, MLP),
model/Compressor/layers.py:26-42 (the learned prior rows).  Scope: the decoder with the encoder frozen, as train.ScoreTrainStep trains the
Score with ConditionNet frozen: `backward` fills the `.grad` of `init_set.prior`, `output.*` and, per level, `decoder[l].ln.*` and
`decoder[l].att1.{fc_q, fc_kv, fc_o, norm1, norm2, mlp.fc.0.0, mlp.out}.*`, and returns the gradient with respect to the latents
(`d_eps`), which is where the posterior / encoder backward will start.  It touches no other parameter: `decoder[l].att`, `decoder[l].prior`,
the encoder, the grouper, the position embedding and ActNorm are the posterior side.

Kernels: the forward's are the inference kernels, unfused; every GEMM of the backward is `ldt_gemm_bf16` on operands prepared by
`ldt_transpose_cast_bf16` (the fp32 linears on the T latent tokens: `ldt_sgemm`); the affine LayerNorm backward is
`ldt_layernorm_modulate_bwd` with the affine read as a modulation shared by all rows (scale = gamma - 1, shift = beta, one "sample" of M
rows: dscale = dgamma, dshift = dbeta); the attention backward is `ldt_attention_bwd_long` (N queries on T keys); the prior rows' gradient is
`ldt_rows_gather_sum`.
"""
import torch

from . import _lib, ops
from ._lib import EPI_BF16, EPI_F32, EPI_RESID_F32
from .layers import conv_w
from .train import _grad2d, _t

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
        if not (torch.is_tensor(eps) and eps.is_cuda):
            raise RuntimeError("DecoderTrainStep.forward: eps is on %s; the HIP path has no CPU fallback"
                               % (eps.device if torch.is_tensor(eps) else type(eps).__name__,))
        self.saved = None
        B, T, Z = eps.shape
        L, z, C, H = m.n_layers, m.z_dim, m.hidden_dim, m.num_heads
        if Z != L * z:
            raise ValueError("DecoderTrainStep.forward: eps %s is not (B, tokens, n_layers * z_dim = %d)" % (tuple(eps.shape), L * z))
        N = m.outsize if num_points is None else int(num_points)
        refuse_undecodable(m, N, T)
        if keep_mask is None:
            keep_mask = m._presence(B, N)
        if keep_mask is not None:
            keep_mask = keep_mask.to(torch.bool)
            if tuple(keep_mask.shape) != (B, m.max_outputs) or not bool((keep_mask.sum(1) == N).all()):
                raise ValueError("DecoderTrainStep.forward: keep_mask must be (B = %d, max_outputs = %d) with %d kept rows per sample"
                                 % (B, m.max_outputs, N))
        P = m.packed()
        M = B * N
        e2 = eps.detach().float().contiguous().view(B * T, Z)
        # which row of each sample every prior row became (ldt_rows_gather_sum's map), built once here where the mask is
        src = ops.prior_row_map(torch.ones((B, N), dtype=torch.bool) if keep_mask is None else keep_mask)
        S = {"B": B, "N": N, "T": T, "eps": e2, "src": src.to(eps.device), "w_zkv_t": [None] * L, "levels": []}
        X = m._initial_set(P, B, N, keep_mask).clone()                  # fp32 [M, C]: the residual stream, updated in place below
        for j in range(L):                                              # reversed(self.decoder), Network.py:263
            Pd = P["dec"][L - 1 - j]
            A = Pd["att1"]
            sb = {"x1": X.clone()}
            sb["h"] = ops.layernorm_modulate(X, w=A["n1"][0], b=A["n1"][1])
            sb["q"] = ops.gemm_bf16(sb["h"], A["wq"], A["bq"], EPI_BF16)
            sb["kv"] = ops.sgemm(e2[:, z * j: z * (j + 1)], Pd["w_zkv"], Pd["b_zkv"], out_bf16=True)      # [B T, 2 C] = K | V, composed linear
            S["w_zkv_t"][j] = _t(Pd["w_zkv"])                                                             # [z, 2 C]: d_eps_j = dkv W_zkv
            sb["o"] = ops.attention_fwd(sb["q"], sb["kv"][:, :C], sb["kv"][:, C:], B, H, N, T, HEAD_DIM)  # [B, H, N, 32] == (M, C) raw view (Q1)
            ops.gemm_bf16(sb["o"].view(M, C), A["wo"], A["bo"], EPI_RESID_F32, out=X, resid=X)
            sb["x2"] = X.clone()
            sb["h2"] = ops.layernorm_modulate(X, w=A["n2"][0], b=A["n2"][1])
            sb["u"] = ops.gemm_bf16(sb["h2"], A["wup"], A["bup"], EPI_BF16)                               # MLP pre-activation
            sb["ug"] = sb["u"].clone()
            ops.block_activation_(sb["ug"], 1)                                                            # GELU
            ops.gemm_bf16(sb["ug"], A["wdn"], A["bdn"], EPI_RESID_F32, out=X, resid=X)
            S["levels"].append(sb)
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
        f32 = lambda t: t.detach().float().contiguous()
        wt = lambda mod_: ops.transpose_cast_bf16(conv_w(mod_).detach())                      # W[N, K] -> bf16 [K, pad64(N)], rebuilt every step

        def linear_bwd(layer, dy, x_in, want_dx=True, epilogue=EPI_F32):
            """dW, db into the layer's .grad; -> dX = dy @ W (dy bf16 [M, n] or fp32; x_in the forward's operand)."""
            ops.wgrad(dy, x_in, out=_grad2d(layer.weight))
            ops.colsum(dy, out=layer.bias.grad)
            if not want_dx:
                return None
            dyb = dy if dy.dtype == torch.bfloat16 and dy.shape[1] % 64 == 0 else ops.cast_pad_bf16(dy, ops.pad64(dy.shape[1]))
            return ops.dgrad(dyb, wt(layer), epilogue)

        def affine_ln_bwd(norm, x, dy, dx):
            """h = LN(x) gamma + beta: dx += the LayerNorm gradient, dgamma and dbeta into the norm's .grad."""
            w, b = norm.affine
            ops.layernorm_modulate_bwd(x, dy, dx, scale=ops.add_f32(f32(w), torch.full_like(w, -1.0)).view(1, C), mod_sample_stride=0,
                                       rows_per_sample=M, dshift=b.grad.view(1, C), dscale=w.grad.view(1, C))

        # output conv C -> 3 (fp32 on both sides of a 3-wide linear)
        d2 = dset.detach().float().contiguous().view(M, 3)
        ops.wgrad(d2, S["xf"], out=_grad2d(m.output.weight))
        ops.colsum(d2, out=m.output.bias.grad)
        dX = ops.sgemm(d2, _t(f32(conv_w(m.output))))                   # [M, C] fp32: the gradient of the residual stream
        d_eps = torch.empty((B * T, L * z), dtype=torch.float32, device=dX.device)
        for j in reversed(range(L)):
            d = m.decoder[L - 1 - j]
            blk, sb = d.att1, S["levels"][j]
            # x = x2 + mlp.out(GELU(mlp.fc(LN2(x2))))                                              (layers.py:226)
            dug = linear_bwd(blk.mlp.out, dX, sb["ug"])
            du = ops.gelu_bwd(sb["u"], dug)
            dh2 = linear_bwd(blk.mlp.fc[0][0], du, sb["h2"])
            affine_ln_bwd(blk.norm2, sb["x2"], dh2, dX)
            # x2 = x1 + fc_o(attention(fc_q(LN1(x1)), fc_kv(ln(eps_j))))                            (layers.py:225, 183-200)
            do = linear_bwd(blk.fc_o, dX, sb["o"].view(M, C), epilogue=EPI_BF16)                  # [M, C] == dO [B, H, N, 32] raw (Q1)
            kv = sb["kv"]
            dkv = torch.empty((B * T, 2 * C), dtype=torch.bfloat16, device=dX.device)             # [dk | dv]
            dq, _, _ = ops.attention_bwd_long(sb["q"], kv[:, :C], kv[:, C:], sb["o"], do, B, H, N, T, dkv_out=dkv)
            dh = linear_bwd(blk.fc_q, dq, sb["h"])
            affine_ln_bwd(blk.norm1, sb["x1"], dh, dX)
            # kv = eps_j W_zkv^T + b_zkv with W_zkv = W_kv W_ln, b_zkv = W_kv b_ln + b_kv: the composed linear hands its gradient to both factors
            e_j = S["eps"][:, z * j: z * (j + 1)]
            dkv32 = ops.widen_bf16(dkv)
            w_kv, w_ln, b_ln = f32(conv_w(blk.fc_kv)), f32(conv_w(d.ln)), f32(d.ln.bias)
            dW_zkv = ops.sgemm(_t(dkv32), _t(e_j))                                                # [2 C, z]
            db_zkv = ops.colsum(dkv32)                                                            # [2 C]
            ops.sgemm(torch.cat([dW_zkv, db_zkv[:, None]], 1), torch.cat([w_ln, b_ln[:, None]], 1), out=_grad2d(blk.fc_kv.weight))   # dW_zkv W_ln^T + db_zkv (x) b_ln
            blk.fc_kv.bias.grad.copy_(db_zkv)
            w_kv_t = _t(w_kv)                                                                     # [C, 2 C]
            ops.sgemm(w_kv_t, _t(dW_zkv), out=_grad2d(d.ln.weight))                               # W_kv^T dW_zkv  [C, z]
            ops.sgemm(db_zkv.view(1, 2 * C), w_kv_t, out=d.ln.bias.grad.view(1, C))               # W_kv^T db_zkv
            ops.sgemm(dkv32, S["w_zkv_t"][j], out=d_eps[:, z * j: z * (j + 1)])                   # dkv W_zkv
        # the learned prior rows: every sample started from them (all, or its kept ones packed to the front)
        m.init_set.prior.grad.copy_(ops.rows_gather_sum(dX, S["src"], N))
        self.d_eps = d_eps.view(B, T, L * z)
        return self.d_eps
