"""Host-side orchestration of one Set-Transformer `ResidualBlock` (reference model/layers.py:183-229) on the
HIP kernels — used by the Compressor (d=128, 4 heads x 32).  The Score network has its own C++
orchestrator (`ldt_score_forward`) because it runs 24 blocks x 1000 steps.

    AdaLN block (Encoder, c = pos embedding):  x += g1 * Attn(mod(LN(x)), y) ; x += g2 * MLP(mod(LN(x)))
    plain block (Decoder, c = None):           x += Attn(LN_affine(x), y)    ; x += MLP(LN_affine(x))

K/V source y (quirk Q2): None -> the normalised/modulated x itself; otherwise the RAW tensor given.
Head merge (quirk Q1): the attention kernel writes [B][H][N][Dh]; that buffer *is* the (B,N,C) raw reinterpret.
A block is four stages (`_modulation_rows`, `_q_kv`, `_attention`, `_mlp`); each of the last three is one fused kernel or the chain of
kernels it stands for, chosen by shape alone (the `_can_*` predicates; the routes per block form: DESIGN.md §4.4).
"""
import collections

import torch

from . import ops
from ._lib import ACT_SILU, EPI_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_F32, block_act_id
from .layers import conv_w


def _bf(w):
    w = w.detach().float().contiguous()
    return ops.cast_pad_bf16(w, ops.pad64(w.shape[1]))


def pack_block(blk):
    """bf16 operand panels + fp32 vectors of one ResidualBlock holder."""
    C, Co = blk.dim_in, blk.dim_out
    wkv = conv_w(blk.fc_kv)
    P = {
        "C": C, "Co": Co, "H": blk.num_heads,
        "wq": _bf(conv_w(blk.fc_q)), "bq": blk.fc_q.bias.detach().float().contiguous(),
        "wkv": _bf(wkv), "bkv": blk.fc_kv.bias.detach().float().contiguous(),
        "wo": _bf(conv_w(blk.fc_o)), "bo": blk.fc_o.bias.detach().float().contiguous(),
        "wup": _bf(conv_w(blk.mlp.fc[0][0])), "bup": blk.mlp.fc[0][0].bias.detach().float().contiguous(),
        "wdn": _bf(conv_w(blk.mlp.out)), "bdn": blk.mlp.out.bias.detach().float().contiguous(),
        "n1": tuple(None if p is None else p.detach().float().contiguous() for p in blk.norm1.affine),
        "n2": tuple(None if p is None else p.detach().float().contiguous() for p in blk.norm2.affine),
        "act": block_act_id(getattr(blk, "act", None)),             # activation behind the norms of the no-condition branch (0 = Identity)
        "norm": getattr(blk.norm1, "kind", "layer_norm"),            # layer_norm | group_norm | None (tools/utils.py:168-181)
        "groups": (getattr(blk.norm1, "num_groups", 0), getattr(blk.norm2, "num_groups", 0)),
    }
    if C == Co and C in (64, 128) and blk.dim_kv == C:              # fc_q | fc_kv as one operand for the fused LN + linear kernel
        P["wqkv"] = torch.cat([P["wq"], P["wkv"]], 0).contiguous()
        P["bqkv"] = torch.cat([P["bq"], P["bkv"]], 0).contiguous()
    if blk.dim_c is not None and C == Co:
        lin = blk.adaLN[1]
        P["wada"], P["bada"] = lin.weight.detach().float().contiguous(), lin.bias.detach().float().contiguous()
    elif blk.dim_c is not None:                                      # U-Net down block: two adaLN heads + conv shortcut
        P["wada1"], P["bada1"] = (t.detach().float().contiguous() for t in (blk.adaLN1[1].weight, blk.adaLN1[1].bias))
        P["wada2"], P["bada2"] = (t.detach().float().contiguous() for t in (blk.adaLN2[1].weight, blk.adaLN2[1].bias))
        P["wsc"], P["bsc"] = _bf(conv_w(blk.shortcut)), blk.shortcut.bias.detach().float().contiguous()
    return P


def apply_norm(kind, x, B, N, affine=(None, None), groups=0, shift=None, scale=None, mod_sample_stride=0, rows_per_sample=0):
    """norm(x) [* w + b] then modulate (layers.py:136-137) -> bf16, for the three norms get_norm builds (tools/utils.py:168-181):
    layer_norm (the LayerNorm kernel; affine only when the block has no condition), group_norm (statistics per sample and group over
    C / G channels x the sample's N tokens — the reference applies nn.GroupNorm to the channels-first (B, C, N) tensor — always affine),
    None (identity).  x: token-major fp32 [B*N, C]."""
    if kind == "layer_norm":
        kw = dict(shift=shift, scale=scale, mod_sample_stride=mod_sample_stride, rows_per_sample=rows_per_sample) if shift is not None else {}
        return ops.layernorm_modulate(x, w=affine[0], b=affine[1], **kw)
    stats = ops.group_stats(x, B, N, groups) if kind == "group_norm" else None
    w, b = affine if kind == "group_norm" else (None, None)
    return ops.norm_apply(x, stats=stats, rows_per_stat=N, w=w, b=b, shift=shift, scale=scale, mod_sample_stride=mod_sample_stride,
                          rows_per_sample=rows_per_sample if shift is not None else 1)


# What a block form hands to its stages.  n1 / n2: the keyword set of norm 1 / norm 2 as the fused LN kernels name it — the affine (ln_w, ln_b:
# None in a conditioned LayerNorm block) and, in the two AdaLN forms, the shift / scale rows, their sample stride and the rows per sample;
# g1 / g2: the gate rows (None: plain form), gate_stride apart per sample; act: the plain form's activation behind both norms (0: none).
_Rows = collections.namedtuple("_Rows", "n1 n2 g1 g2 gate_stride act")


def _modulation_rows(P, c, rps):
    C, Co = P["C"], P["Co"]
    n1, n2 = dict(ln_w=P["n1"][0], ln_b=P["n1"][1]), dict(ln_w=P["n2"][0], ln_b=P["n2"][1])
    if c is None:                                                                   # plain form (layers.py:224-226)
        return _Rows(n1, n2, None, None, 0, P.get("act", 0))
    if C == Co:                                                                     # AdaLN, layers.py:214
        mod = ops.sgemm(c, P["wada"], P["bada"], act_in=ACT_SILU)                  # [B, 6C]
        sh1, sc1, g1, sh2, sc2, g2 = (mod[:, i * C:(i + 1) * C] for i in range(6))
        s1 = s2 = 6 * C
    else:                                                                           # U-Net down, layers.py:216-217
        m1 = ops.sgemm(c, P["wada1"], P["bada1"], act_in=ACT_SILU)                 # [B, 2C]   shift_msa | scale_msa
        mod = ops.sgemm(c, P["wada2"], P["bada2"], act_in=ACT_SILU)                # [B, 4Co]  gate_msa | shift_mlp | scale_mlp | gate_mlp
        sh1, sc1, s1, s2 = m1[:, :C], m1[:, C:], 2 * C, 4 * Co
        g1, sh2, sc2, g2 = (mod[:, i * Co:(i + 1) * Co] for i in range(4))
    n1.update(shift=sh1, scale=sc1, mod_sample_stride=s1, rows_per_sample=rps)
    n2.update(shift=sh2, scale=sc2, mod_sample_stride=s2, rows_per_sample=rps)
    return _Rows(n1, n2, g1, g2, s2, 0)


def _norm_chain(P, i, x, B, N, act, ln_w, ln_b, **mod):
    """Norm i (0, 1) of the block by the norm kernels, then the block activation in an element-wise pass -> bf16 rows."""
    h = apply_norm(P.get("norm", "layer_norm"), x, B, N, (ln_w, ln_b), P["groups"][i], **mod)
    return ops.block_activation_(h, act) if act else h


def _ln_fusable(P, R, x):
    """Both fused LN kernels are LayerNorm kernels without an activation slot, and read the rows of x as float4."""
    return P.get("norm", "layer_norm") == "layer_norm" and not R.act and x.stride(0) % 4 == 0


def _can_ln_linear(P, R, x):
    """ldt_ln_linear: C in {64, 128} (so W has no padded columns) and N % 64 == 0."""
    return _ln_fusable(P, R, x) and P["C"] in (64, 128) and P["wq"].shape[1] == P["C"] and P["Co"] % 64 == 0


def _q_kv(P, R, x, B, Nq, y_bf16, Nk, kv_pre, q_pre):
    """-> (q, K | V bf16 [B*Nk, 2Co] (layers.py:189), Nk).  LN1 (+ modulate | affine) + fc_q [+ fc_kv on the same normalised input] in ONE kernel
    (csrc/fused_mlp.hip: the normalised rows are never written), or q_pre from the previous block's MLP kernel; or norm, activation, GEMMs."""
    ext = y_bf16 is not None or kv_pre is not None                                  # K/V come from another tensor
    if not _can_ln_linear(P, R, x):
        h = _norm_chain(P, 0, x, B, Nq, R.act, **R.n1)
        q = ops.gemm_bf16(h, P["wq"], P["bq"], EPI_BF16)
        if not ext:
            y_bf16, Nk = h, Nq
    elif not ext and "wqkv" in P:
        qkv = ops.ln_linear(x, P["wqkv"], P["bqkv"], **R.n1)
        return qkv[:, :P["Co"]], qkv[:, P["Co"]:], Nq
    else:
        q = q_pre if (q_pre is not None and ext) else ops.ln_linear(x, P["wq"], P["bq"], **R.n1)
        if not ext:                                  # a U-Net down block at hidden 64 (C = 128, Co = 64, so no wqkv): LN runs twice
            y_bf16, Nk = _norm_chain(P, 0, x, B, Nq, 0, **R.n1), Nq
    return q, (kv_pre if kv_pre is not None else ops.gemm_bf16(y_bf16, P["wkv"], P["bkv"], EPI_BF16)), Nk


def _can_attention_oproj(P, R, Nq, per_token):
    """ldt_attention_oproj_resid: Dh = 32 with H in {2, 4}, Nq % H == 0 (the raw head merge, Q1), dense Wo, one gate row per SAMPLE."""
    Co, H = P["Co"], P["H"]
    return Co // H == 32 and H in (2, 4) and Nq % H == 0 and P["wo"].shape == (Co, Co) and not (per_token and R.g1 is not None)


def _attention(P, R, x, q, kv, B, Nq, Nk, rps, per_token):
    """x += g1 * fc_o(Attn(q, K, V)) -> x (a new tensor behind the conv shortcut of a U-Net down block).  Attention + out-projection + gated
    residual in ONE kernel (csrc/attention.hip, OPROJ: the [B,H,Nq,Dh] result never goes to HBM), or attention and the residual GEMM."""
    C, Co, H = P["C"], P["Co"], P["H"]
    if C != Co:                                                                     # shortcut(x): Conv1d dim_in -> dim_out
        x = ops.gemm_bf16(ops.cast_pad_bf16(x, ops.pad64(C)), P["wsc"], P["bsc"], EPI_F32)
    if _can_attention_oproj(P, R, Nq, per_token):
        ops.attention_oproj_resid_(q, kv[:, :Co], kv[:, Co:], B, H, Nq, Nk, 32, P["wo"], P["bo"], x, gate=R.g1, gate_sample_stride=R.gate_stride)
    else:
        a = ops.attention_fwd(q, kv[:, :Co], kv[:, Co:], B, H, Nq, Nk, Co // H)     # [B,H,Nq,Dh] == (B*Nq, Co) raw view
        ops.gemm_bf16(a.view(B * Nq, Co), P["wo"], P["bo"], EPI_RESID_F32, out=x, resid=x, gate=R.g1, gate_sample_stride=R.gate_stride,
                      rows_per_sample=rps)
    return x


def _can_ln_mlp(P, R, x):
    """ldt_ln_mlp_resid: C in {64, 128} with dense W_up [4C][C] (mlp_ratio 4)."""
    return _ln_fusable(P, R, x) and P["Co"] in (64, 128) and P["wup"].shape == (4 * P["Co"], P["Co"])


def _can_next_linear(P, next_P):
    """ldt_ln_mlp_resid_next: a next block of the same width, dense W [C][C] with N % 64 == 0, and an affine LayerNorm (a plain block)."""
    Co = P["Co"]
    return next_P is not None and next_P["C"] == next_P["Co"] == Co and tuple(next_P["wq"].shape) == (Co, Co) and Co % 64 == 0 \
        and next_P["n1"][0] is not None


def _mlp(P, R, x, B, Nq, rps, x_bf16_out, next_P):
    """x += g2 * MLP(norm2(x)) in place -> q_next, or None without the hand-off.  LN2 + MLP + gated residual in ONE pass over x
    (csrc/fused_mlp.hip), which also stores x_bf16_out and the next block's LN1 + fc_q; or norm, activation, two GEMMs, one cast."""
    if _can_ln_mlp(P, R, x):
        nxt = dict(w=next_P["wq"], bias=next_P["bq"], ln_w=next_P["n1"][0], ln_b=next_P["n1"][1]) if _can_next_linear(P, next_P) else None
        r = ops.ln_mlp_resid_(x, P["wup"], P["bup"], P["wdn"], P["bdn"], gate=R.g2, x_bf16_out=x_bf16_out, next_linear=nxt, **R.n2)
        return r[1] if nxt is not None else None
    h2 = _norm_chain(P, 1, x, B, Nq, R.act, **R.n2)
    u = ops.gemm_bf16(h2, P["wup"], P["bup"], EPI_GELU_BF16)
    ops.gemm_bf16(u, P["wdn"], P["bdn"], EPI_RESID_F32, out=x, resid=x, gate=R.g2, gate_sample_stride=R.gate_stride, rows_per_sample=rps)
    if x_bf16_out is not None:
        x_bf16_out.copy_(ops.cast_pad_bf16(x, x_bf16_out.shape[1]))


def _block(P, x, B, Nq, y_bf16, Nk, c, per_token, x_bf16_out, kv_pre, q_pre=None, next_P=None):
    rps = 1 if per_token else Nq                                                    # rows that share one modulation row
    R = _modulation_rows(P, c, rps)
    q, kv, Nk = _q_kv(P, R, x, B, Nq, y_bf16, Nk, kv_pre, q_pre)
    x = _attention(P, R, x, q, kv, B, Nq, Nk, rps, per_token)
    return x, _mlp(P, R, x, B, Nq, rps, x_bf16_out, next_P)


def residual_block(P, x, B, Nq, y_bf16=None, Nk=None, c=None, per_token=False, x_bf16_out=None, kv_pre=None):
    """x fp32 [B*Nq, C] updated IN PLACE (and returned) when dim_out == dim_in; a NEW [B*Nq, dim_out] tensor is returned
    for a U-Net down block.  y_bf16: raw K/V source [B*Nk, Ckv] (bf16) or None (self, modulated).
    c: fp32 [B, dim_c] condition (AdaLN) — or [B*Nq, dim_c] with per_token=True (layers.py:210: a (B, dim_c, N) condition
    modulates every token with its own row; the Compressor's `pos_embedding: mlp`) — or None (plain LayerNorm block).
    x_bf16_out: optional bf16 [B*Nq, dim_out] buffer that receives a copy of the block's result (written by the fused MLP
    kernel's own store pass, or by one cast on the unfused path).
    kv_pre: bf16 [B*Nk, 2*dim_out] = fc_kv(y) computed by the caller (then y_bf16 is not needed: pass Nk)."""
    return _block(P, x, B, Nq, y_bf16, Nk, c, per_token, x_bf16_out, kv_pre)[0]


def residual_block_handoff(P, x, B, Nq, Nk, kv_pre, q_pre=None, next_P=None, c=None, x_bf16_out=None):
    """A decoder level's block: `residual_block` on the caller's K | V (`kv_pre`) that hands the next level its query projection -> (x, q_next).
    next_P: packed holder of the plain-LayerNorm block that will run next on the same rows with a K/V source of its own: its LN1 + fc_q is
    computed by THIS block's last kernel; q_next is None where the shapes do not allow it.  q_pre: the previous level's q_next, or None."""
    return _block(P, x, B, Nq, None, Nk, c, False, x_bf16_out, kv_pre, q_pre, next_P)


def pack_final(fl):
    lin = fl.adaLN[1]
    return {"C": fl.ln.in_channels, "w": _bf(conv_w(fl.ln)), "b": fl.ln.bias.detach().float().contiguous(),
            "n_out": fl.ln.out_channels, "norm": getattr(fl.norm, "kind", "layer_norm"), "groups": getattr(fl.norm, "num_groups", 0),
            "n": tuple(None if p is None else p.detach().float().contiguous() for p in fl.norm.affine),
            "wada": lin.weight.detach().float().contiguous(), "bada": lin.bias.detach().float().contiguous()}


def final_layer(P, x, B, N, c, out_dtype=torch.float32, per_token=False):
    """FinalLayer with condition (layers.py:240-246): Conv(mod(LN(x))); c [B, dim_c], or [B*N, dim_c] with per_token."""
    C = P["C"]
    mod = ops.sgemm(c, P["wada"], P["bada"], act_in=ACT_SILU)                      # [B, 2C] shift | scale
    h = apply_norm(P.get("norm", "layer_norm"), x, B, N, P.get("n", (None, None)), P.get("groups", 0), shift=mod[:, :C], scale=mod[:, C:],
                   mod_sample_stride=2 * C, rows_per_sample=1 if per_token else N)
    return ops.gemm_bf16(h, P["w"], P["b"], EPI_F32 if out_dtype == torch.float32 else EPI_BF16, n=P["n_out"])
