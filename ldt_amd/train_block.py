"""The transformer block of the training steps, forward and backward, written once, and the small pieces the
steps share around it: the FinalLayer, the backward of a bf16 linear, of the affine LayerNorm and of the stacked adaLN linear.

Reference: model/layers.py:183-229 (ResidualBlock: LayerNorm -> q / K | V -> attention -> fc_o + residual -> LayerNorm -> MLP-up -> GELU ->
MLP-down + residual), :240-246 (FinalLayer).  `block_fwd` runs the inference kernels unfused and keeps every operand of the backward;
`block_bwd` walks it back: every GEMM is `ldt_gemm_bf16` on operands prepared by `ldt_transpose_cast_bf16`, everything else is
csrc/score_bwd.hip and the attention backward entry the caller names.  What varies between train.ScoreTrainStep and the three steps of
compressor_train is an argument: the norm / gate form (`mod`), where q and K | V come from (`y`, `kv`), the attention geometry.

`TrainBlock(ops)` binds these pieces to the kernels of the step that runs them: a step hands over its own module's `ops`, so whatever
stands in for a step module's `ops` (a recording proxy, a planted fault) sees the block's calls too; without an argument it is this
module's attribute `ops`.
"""
import torch

from . import ops
from ._lib import EPI_BF16, EPI_F32, EPI_RESID_F32
from .layers import conv_w


def _t(x):
    """fp32 transpose as a dense matrix (data movement only: ldt_sgemm takes row strides, not column strides).  Copied into a fresh
    tensor: `.t().contiguous()` hands a one-row matrix back as it is ([1, n] -> [n, 1] with strides (1, n) counts as contiguous), and
    ops.sgemm refuses its last-dim stride — a batch of one sample could not take a step."""
    return x.new_empty((x.shape[1], x.shape[0])).copy_(x.t())


def _grad2d(p):
    return p.grad.view(p.shape[0], -1)


def refuse_host(where, what, *tensors):
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("%s: %s is on %s; the HIP path has no CPU fallback" % (where, what, t.device if torch.is_tensor(t) else type(t).__name__))


class ModRows:
    """The AdaLN form's operands: the per-sample modulation rows `mod` fp32 [B, n_mod] (and, for a backward, their gradient `dmod`) as
    the kernels take them — v(off) / d(off) the D-wide column block at `off`, kw / gk the stride keywords of a modulation / a gate."""

    def __init__(self, mod, D, T, dmod=None):
        self.D = D
        self.v = lambda off: mod[:, off:off + D]
        self.d = lambda off: dmod[:, off:off + D]
        self.kw = dict(mod_sample_stride=mod.shape[1], rows_per_sample=T)
        self.gk = dict(gate_sample_stride=mod.shape[1], rows_per_sample=T)


class TrainBlock:
    def __init__(self, step_ops=None):
        self.ops = ops if step_ops is None else step_ops

    # ---------------------------------------------------------------- backward of the linears and the affine LayerNorm
    def linear_bwd(self, layer, dy, x_in, want_dx=True, epilogue=EPI_F32):
        """dW, db into the layer's .grad views; -> dX = dy @ W (dy bf16 [M, N] or fp32; x_in the forward's operand)."""
        ops = self.ops
        ops.wgrad(dy, x_in, out=_grad2d(layer.weight))
        ops.colsum(dy, out=layer.bias.grad)
        if not want_dx:
            return None
        dyb = dy if dy.dtype == torch.bfloat16 and dy.shape[1] % 64 == 0 else ops.cast_pad_bf16(dy.float() if dy.dtype != torch.float32 else dy,
                                                                                               ops.pad64(dy.shape[1]))
        return ops.dgrad(dyb, ops.transpose_cast_bf16(conv_w(layer).detach()), epilogue)  # W[N, K] -> bf16 [K, pad64(N)], rebuilt every step

    def affine_ln_bwd(self, norm, x, dy, dx):
        """h = LN(x) gamma + beta: dx += the LayerNorm gradient, dgamma and dbeta into the norm's .grad.  The affine is read as a modulation
        shared by all rows (scale = gamma - 1, shift = beta, one "sample" of M rows: dscale = dgamma, dshift = dbeta)."""
        w, b = norm.affine
        M, C = x.shape
        scale = self.ops.add_f32(w.detach().float().contiguous(), torch.full_like(w, -1.0)).view(1, C)
        self.ops.layernorm_modulate_bwd(x, dy, dx, scale=scale, mod_sample_stride=0, rows_per_sample=M, dshift=b.grad.view(1, C),
                                        dscale=w.grad.view(1, C))

    def adaln_bwd(self, dmod, w_ada, c, lins):
        """mod = adaLN.1(SiLU(c)) for every block and FinalLayer, one fp32 linear on transposed operands with its rows stacked in the order
        of `lins`: each layer's .grad is filled from its rows; -> dc fp32 [B, c_dim]."""
        ops = self.ops
        ds = ops.sgemm(dmod, _t(w_ada))                                                    # d SiLU(c)
        dc, s_c = ops.silu_bwd(c, ds, want_act=True)
        dW = ops.sgemm(_t(dmod), _t(s_c))                                                  # [n_mod, c_dim]
        db = ops.colsum(dmod)
        r = 0
        for lin in lins:
            n = lin.weight.shape[0]
            lin.weight.grad.copy_(dW[r:r + n])
            lin.bias.grad.copy_(db[r:r + n])
            r += n
        return dc

    # ---------------------------------------------------------------- the norm and the residual in their two forms
    def _ln_fwd(self, X, affine, mod, off):
        if mod is None:
            return self.ops.layernorm_modulate(X, w=affine[0], b=affine[1])
        return self.ops.layernorm_modulate(X, shift=mod.v(off), scale=mod.v(off + mod.D), **mod.kw)

    def _ln_bwd(self, norm, x, dy, dx, mod, off):
        if mod is None:
            self.affine_ln_bwd(norm, x, dy, dx)
        else:
            self.ops.layernorm_modulate_bwd(x, dy, dx, scale=mod.v(off + mod.D), dshift=mod.d(off), dscale=mod.d(off + mod.D), **mod.kw)

    def _residual_fwd(self, sb, key, a_in, w, b, X, mod, off):
        """X += [gate *] (a_in @ w^T + b); under a gate the bf16 branch output is kept as sb[key] for dgate, by a GEMM of its own."""
        if mod is None:
            self.ops.gemm_bf16(a_in, w, b, EPI_RESID_F32, out=X, resid=X)
        else:
            sb[key] = self.ops.gemm_bf16(a_in, w, b, EPI_BF16)
            self.ops.gemm_bf16(a_in, w, b, EPI_RESID_F32, out=X, resid=X, gate=mod.v(off), **mod.gk)

    def _residual_bwd(self, dX, sb, key, mod, off):
        """-> the gradient of the branch output: dX itself, or bf16 dX * gate with dgate written into its dmod columns."""
        if mod is None:
            return dX
        return self.ops.gate_residual_bwd(dX, mod.v(off), sb[key], dgate=mod.d(off), **mod.gk)[0]

    # ---------------------------------------------------------------- the block
    def block_fwd(self, A, X, geom, mod=None, m0=0, y=None, kv=None, kv_bwd=None):
        """One ResidualBlock on the fp32 rows X [B Nq, C], updated in place; unfused, every operand of the backward kept -> the block's tape.
        A: the block's bf16 panels and fp32 biases under blocks.pack_block's names.  geom = (B, H, Nq, Nk, head_dim).
        mod: None for the affine form (LayerNorm with A["n1"] / A["n2"], no gate), or the ModRows of the AdaLN form, the block's six column
          blocks (shift, scale, gate of the attention half, then of the MLP half) starting at m0; a1 / a2 are then kept for dgate.
        q and K | V: with neither y nor kv, one GEMM on the packed q | k | v panel A["wqkv"] of h, kept as `qkv` (self-attention); with y, q
          from h and K | V = fc_kv(y) — y bf16 rows, or the fp32 stream X itself, cast here behind the norm and kept as `y` (K / V from the
          RAW x, quirk Q2); with kv bf16 [B Nk, 2 C], q from h and K | V as given.
        kv_bwd(y, kv) -> the K | V the backward is to read, formed right behind the attention (compressor_train._centred_keys)."""
        ops = self.ops
        B, H, Nq, Nk, hd = geom
        C, M = X.shape[1], B * Nq
        sb = {"x1": X.clone()}
        sb["h"] = self._ln_fwd(X, A.get("n1"), mod, m0)
        if y is None and kv is None:
            sb["qkv"] = ops.gemm_bf16(sb["h"], A["wqkv"], A["bqkv"], EPI_BF16)
            q, kv = sb["qkv"][:, :C], sb["qkv"][:, C:]
        else:
            if y is not None and y.dtype == torch.float32:
                y = sb["y"] = ops.cast_pad_bf16(y, ops.pad64(C))
            q = sb["q"] = ops.gemm_bf16(sb["h"], A["wq"], A["bq"], EPI_BF16)
            sb["kv"] = kv = ops.gemm_bf16(y, A["wkv"], A["bkv"], EPI_BF16) if y is not None else kv      # [B Nk, 2 C] = K | V
        sb["o"] = ops.attention_fwd(q, kv[:, :C], kv[:, C:], B, H, Nq, Nk, hd)                            # [B, H, Nq, Dh] == (M, C) raw view (Q1)
        if kv_bwd is not None:
            sb["kv"] = kv_bwd(y, kv)
        self._residual_fwd(sb, "a1", sb["o"].view(M, C), A["wo"], A["bo"], X, mod, m0 + 2 * C)
        sb["x2"] = X.clone()
        sb["h2"] = self._ln_fwd(X, A.get("n2"), mod, m0 + 3 * C)
        sb["u"] = ops.gemm_bf16(sb["h2"], A["wup"], A["bup"], EPI_BF16)                                   # MLP pre-activation
        sb["ug"] = sb["u"].clone()
        ops.block_activation_(sb["ug"], 1)                                                                # GELU
        self._residual_fwd(sb, "a2", sb["ug"], A["wdn"], A["bdn"], X, mod, m0 + 5 * C)
        return sb

    def block_bwd(self, blk, sb, dX, geom, attention_bwd=None, mod=None, m0=0, y=None, dy_sum=None):
        """Backward of block_fwd: dX fp32 [B Nq, C], the gradient of the block's result, becomes the gradient of its input; the block's
        .grads and, under AdaLN, its columns of dmod are filled.  attention_bwd: the ops entry for (Nq, Nk) of a block with K | V of its
        own (attention_bwd_cross, _long or _wide); the fused q | k | v form runs ops.attention_bwd.
        -> None for the fused form; dkv bf16 [B Nk, 2 C] = dK | dV for a block whose K | V the caller made; with y, the operand of fc_kv,
        fc_kv's backward runs here, ahead of norm1's, and dy fp32 [B Nk, C] is returned for the caller to add into the stream y came from
        (added to dy_sum first when one is given: the Score's running sum over its cross blocks)."""
        ops, linear_bwd = self.ops, self.linear_bwd
        B, H, Nq, Nk, hd = geom
        C, M = dX.shape[1], B * Nq
        # x = x2 + [gate_mlp *] mlp.out(GELU(mlp.fc(norm2(x2))))                            (layers.py:219, 226)
        dug = linear_bwd(blk.mlp.out, self._residual_bwd(dX, sb, "a2", mod, m0 + 5 * C), sb["ug"])
        du = ops.gelu_bwd(sb["u"], dug)
        dh2 = linear_bwd(blk.mlp.fc[0][0], du, sb["h2"])
        self._ln_bwd(blk.norm2, sb["x2"], dh2, dX, mod, m0 + 3 * C)
        # x2 = x1 + [gate_msa *] fc_o(attention(q, K | V))                                  (layers.py:218, 225, 183-200)
        do = linear_bwd(blk.fc_o, self._residual_bwd(dX, sb, "a1", mod, m0 + 2 * C), sb["o"].view(M, C), epilogue=EPI_BF16)   # [M, C] == dO [B, H, Nq, Dh] raw (Q1)
        if "qkv" in sb:
            qkv = sb["qkv"]
            dqkv = torch.empty((M, 3 * C), dtype=torch.bfloat16, device=do.device)        # [dq | dk | dv], the dY of fc_q | fc_kv
            dq, _, _ = ops.attention_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], sb["o"], do, B, H, Nq, head_dim=hd, out=dqkv)
            linear_bwd(blk.fc_q, dq, sb["h"], want_dx=False)
            linear_bwd(blk.fc_kv, dqkv[:, C:], sb["h"], want_dx=False)
            wqkv_t = ops.transpose_cast_bf16(torch.cat([conv_w(blk.fc_q), conv_w(blk.fc_kv)], 0).detach())
            dh, ret = ops.dgrad(dqkv, wqkv_t, EPI_F32), None
        else:
            kv = sb["kv"]
            ret = torch.empty((B * Nk, 2 * C), dtype=torch.bfloat16, device=do.device)    # [dk | dv], the dY of fc_kv
            dq, _, _ = attention_bwd(sb["q"], kv[:, :C], kv[:, C:], sb["o"], do, B, H, Nq, Nk, head_dim=hd, dkv_out=ret)
            dh = linear_bwd(blk.fc_q, dq, sb["h"])
            if y is not None:
                ret = linear_bwd(blk.fc_kv, ret, y)
                if dy_sum is not None:
                    ret = ops.add_f32(dy_sum, ret)
        self._ln_bwd(blk.norm1, sb["x1"], dh, dX, mod, m0)
        return ret

    # ---------------------------------------------------------------- FinalLayer (layers.py:240-246)
    def final_fwd(self, X, w, b, n, mod, f0):
        """-> (hf bf16 = mod(LN(X)) with the (shift, scale) column blocks at f0, the fp32 output of the n-wide linear on it)."""
        hf = self._ln_fwd(X, None, mod, f0)
        return hf, self.ops.gemm_bf16(hf, w, b, EPI_F32, n=n)

    def final_bwd(self, lin, d_out, xf, hf, dX, mod, f0):
        """d_out fp32 [M, n]: the linear's .grads, its dmod columns, and dX += the gradient of the stream xf."""
        self._ln_bwd(None, xf, self.linear_bwd(lin, d_out, hf), dX, mod, f0)
