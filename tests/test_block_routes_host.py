"""Which kernels each form of the inference block launches (ldt_amd/blocks.py), held on the CPU.

The golden tests compare a whole forward with the oracle at 1e-4: a block that fell from a fused kernel to its chain would still pass them and
only show as lost speed.  Here `blocks.ops` is replaced by a recording stand-in (in the spirit of tests/train_tape.py): every entry point
returns a tensor of the shape and dtype the real one returns, and the call's name and scalar keywords are recorded.  Real `ResidualBlock`
holders are packed on the CPU through the same stand-in, and each case asserts the ORDERED kernel names plus the facts named with it.

The table below was written by hand from the block as it stood before it was split into stages; it is the contract, not a print-out."""
import inspect

import pytest
import torch

from ldt_amd import _lib, blocks, ops as real_ops
from ldt_amd.layers import ResidualBlock

BF, F32 = torch.bfloat16, torch.float32


class RecordingOps:
    """Stand-in for `ldt_amd.ops` as blocks.py uses it.  calls: [(name, {parameter: value})] with every parameter bound by the real entry
    point's signature (defaults included), so that a keyword passed or left at its default reads the same."""

    def __init__(self):
        self.calls = []

    pad64 = staticmethod(real_ops.pad64)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError("%s: an entry point the stand-in does not know" % name[1:])
        shape_of = getattr(self, "_" + name)
        sig = inspect.signature(getattr(real_ops, name))

        def recorded(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            self.calls.append((name, dict(bound.arguments)))
            return shape_of(**bound.arguments)
        return recorded

    # ---- what each entry point returns (shape, dtype); in-place ones hand back their operand
    @staticmethod
    def _new(t, out, shape, dtype):
        return out if out is not None else torch.zeros(shape, dtype=dtype, device=t.device)

    def _cast_pad_bf16(self, src, cols_pad, out):
        rows = src.numel() // src.shape[-1]
        return self._new(src, out, (rows, cols_pad or (src.shape[-1] + 3) // 4 * 4), BF)

    def _sgemm(self, a, w, bias, act_in, act_out, out, out_bf16):
        assert a.dtype == w.dtype == F32 and a.shape[1] == w.shape[1]
        return self._new(a, out, (a.shape[0], w.shape[0]), BF if out_bf16 else F32)

    def _gemm_bf16(self, x, w, bias, epilogue, out, resid, skip, gate, gate_sample_stride, rows_per_sample, step_ptr, gate_step_stride, n):
        assert x.dtype == w.dtype == BF and x.shape[1] == w.shape[1], (x.shape, w.shape)
        return self._new(x, out, (x.shape[0], n if n is not None else w.shape[0]), F32 if epilogue in (_lib.EPI_F32, _lib.EPI_RESID_F32) else BF)

    def _layernorm_modulate(self, x, out, **kw):
        return self._new(x, out, tuple(x.shape), BF)

    def _norm_apply(self, x, out, **kw):
        return self._new(x, out, tuple(x.shape), BF)

    def _group_stats(self, x, B, T, groups, eps):
        return torch.zeros((B, groups, 2), dtype=F32)

    def _block_activation_(self, x, kind):
        assert x.dtype == BF and kind > 0
        return x

    def _attention_fwd(self, q, k, v, B, H, Nq, Nk, head_dim, out):
        assert q.shape[0] == B * Nq and k.shape[0] == v.shape[0] == B * Nk
        return self._new(q, out, (B, H, Nq, head_dim), BF)

    def _attention_oproj_resid_(self, q, k, v, B, H, Nq, Nk, head_dim, wo, bo, x, gate, gate_sample_stride):
        assert q.shape[0] == B * Nq and k.shape[0] == v.shape[0] == B * Nk and tuple(x.shape) == (B * Nq, H * head_dim)
        return x

    def _ln_linear(self, x, w, out, **kw):
        assert x.dtype == F32 and w.shape[1] == x.shape[1]
        return self._new(x, out, (x.shape[0], w.shape[0]), BF)

    def _ln_mlp_resid_(self, x, next_linear, **kw):
        if next_linear is None:
            return x
        return x, torch.zeros((x.shape[0], next_linear["w"].shape[0]), dtype=BF)


@pytest.fixture
def rec(monkeypatch):
    r = RecordingOps()
    monkeypatch.setattr(blocks, "ops", r)
    return r


C, H, B, NQ, NK, PD = 64, 2, 2, 8, 5, 16            # block width, heads (Dh = 32), samples, query rows, external K/V rows, condition width


def pack(rec, dim_c=None, C=C, H=H, norm="layer_norm", act=None, dim_out=None):
    torch.manual_seed(0)
    P = blocks.pack_block(ResidualBlock(C, C, dim_c, H, norm=norm, dim_out=dim_out, act=act))
    del rec.calls[:]                                # (packing casts the panels through the stand-in too)
    return P


def rows(n=B * NQ, width=C):
    return torch.zeros((n, width), dtype=F32)


def names(rec):
    return [n for n, _ in rec.calls]


def only(rec, name):
    hits = [kw for n, kw in rec.calls if n == name]
    assert len(hits) == 1, "%d calls of %s in %s" % (len(hits), name, names(rec))
    return hits[0]


def test_encoder_adaln_block_kv_from_y(rec):
    P = pack(rec, dim_c=PD)
    x = rows()
    r = blocks.residual_block(P, x, B, NQ, y_bf16=torch.zeros((B * NQ, C), dtype=BF), Nk=NQ, c=torch.zeros((B, PD)))
    assert r is x
    assert names(rec) == ["sgemm", "ln_linear", "gemm_bf16", "attention_oproj_resid_", "ln_mlp_resid_"]
    assert only(rec, "sgemm")["act_in"] == _lib.ACT_SILU
    q = only(rec, "ln_linear")
    assert q["w"] is P["wq"] and q["ln_w"] is None and q["shift"] is not None and (q["mod_sample_stride"], q["rows_per_sample"]) == (6 * C, NQ)
    assert only(rec, "gemm_bf16")["w"] is P["wkv"]
    a = only(rec, "attention_oproj_resid_")
    assert a["gate"] is not None and a["gate_sample_stride"] == 6 * C and a["head_dim"] == 32 and (a["Nq"], a["Nk"]) == (NQ, NQ)
    m = only(rec, "ln_mlp_resid_")
    assert m["gate"] is not None and (m["mod_sample_stride"], m["rows_per_sample"]) == (6 * C, NQ) and m["next_linear"] is None


def test_encoder_adaln_block_per_token(rec):
    P = pack(rec, dim_c=PD)
    blocks.residual_block(P, rows(), B, NQ, y_bf16=torch.zeros((B * NQ, C), dtype=BF), Nk=NQ, c=torch.zeros((B * NQ, PD)), per_token=True)
    # one gate row per token: the fused attention kernel gates per sample, so attention and the gated residual GEMM run apart
    assert names(rec) == ["sgemm", "ln_linear", "gemm_bf16", "attention_fwd", "gemm_bf16", "ln_mlp_resid_"]
    assert only(rec, "ln_linear")["rows_per_sample"] == 1
    resid = rec.calls[4][1]
    assert resid["epilogue"] == _lib.EPI_RESID_F32 and resid["rows_per_sample"] == 1 and resid["gate"] is not None and resid["gate_sample_stride"] == 6 * C
    assert resid["out"] is resid["resid"]
    assert only(rec, "ln_mlp_resid_")["rows_per_sample"] == 1


def _decoder(rec, dim_c=None, **kw):
    P, nxt = pack(rec, dim_c=dim_c), pack(rec, dim_c=dim_c)
    x, xb = rows(), torch.zeros((B * NQ, C), dtype=BF)
    kv = torch.zeros((B * NK, 2 * C), dtype=BF)
    r = blocks.residual_block_handoff(P, x, B, NQ, NK, kv, next_P=nxt, x_bf16_out=xb, **kw)
    assert isinstance(r, tuple) and len(r) == 2 and r[0] is x
    return P, nxt, xb, kv, r[1]


def test_decoder_att1_hands_the_next_query_over(rec):
    P, nxt, xb, kv, q_next = _decoder(rec)
    assert names(rec) == ["ln_linear", "attention_oproj_resid_", "ln_mlp_resid_"]
    q = only(rec, "ln_linear")
    assert q["w"] is P["wq"] and q["ln_w"] is P["n1"][0] and q["ln_b"] is P["n1"][1] and q["shift"] is None
    a = only(rec, "attention_oproj_resid_")
    assert a["gate"] is None and a["gate_sample_stride"] == 0 and a["Nk"] == NK and a["k"].data_ptr() == kv.data_ptr()
    m = only(rec, "ln_mlp_resid_")
    assert m["x_bf16_out"] is xb and m["ln_w"] is P["n2"][0] and m["gate"] is None
    nl = m["next_linear"]
    assert nl["w"] is nxt["wq"] and nl["bias"] is nxt["bq"] and nl["ln_w"] is nxt["n1"][0] and nl["ln_b"] is nxt["n1"][1]
    assert q_next is not None and tuple(q_next.shape) == (B * NQ, C) and q_next.dtype == BF


def test_decoder_att1_takes_the_query_handed_over(rec):
    qp = torch.zeros((B * NQ, C), dtype=BF)
    _, _, _, _, q_next = _decoder(rec, q_pre=qp)
    assert names(rec) == ["attention_oproj_resid_", "ln_mlp_resid_"]
    assert only(rec, "attention_oproj_resid_")["q"] is qp and q_next is not None


def test_decoder_att1_with_label_condition_has_no_handoff(rec):
    # the next level's block is an AdaLN block too: its norm 1 has no affine and its rows are not known yet
    _, _, xb, _, q_next = _decoder(rec, dim_c=PD, c=torch.zeros((B, PD)))
    assert names(rec) == ["sgemm", "ln_linear", "attention_oproj_resid_", "ln_mlp_resid_"]
    assert only(rec, "ln_linear")["shift"] is not None and only(rec, "attention_oproj_resid_")["gate"] is not None
    m = only(rec, "ln_mlp_resid_")
    assert m["next_linear"] is None and m["x_bf16_out"] is xb and q_next is None


def test_posterior_block(rec):
    P = pack(rec)
    y = torch.zeros((B * NK, C), dtype=BF)
    x = rows()
    assert blocks.residual_block(P, x, B, NQ, y_bf16=y, Nk=NK) is x
    assert names(rec) == ["ln_linear", "gemm_bf16", "attention_oproj_resid_", "ln_mlp_resid_"]
    assert only(rec, "ln_linear")["ln_w"] is P["n1"][0] and only(rec, "gemm_bf16")["x"] is y
    assert only(rec, "attention_oproj_resid_")["gate"] is None and only(rec, "attention_oproj_resid_")["Nk"] == NK
    assert only(rec, "ln_mlp_resid_")["ln_w"] is P["n2"][0]


def test_packed_self_attention(rec):
    P = pack(rec, dim_c=PD)
    blocks.residual_block(P, rows(), B, NQ, c=torch.zeros((B, PD)))
    assert names(rec) == ["sgemm", "ln_linear", "attention_oproj_resid_", "ln_mlp_resid_"]
    q = only(rec, "ln_linear")
    assert q["w"] is P["wqkv"] and tuple(q["w"].shape) == (3 * C, C) and q["bias"] is P["bqkv"]
    assert only(rec, "attention_oproj_resid_")["Nk"] == NQ


def test_unet_down_block_128_to_64(rec):
    P = pack(rec, dim_c=PD, C=128, dim_out=64)
    assert "wqkv" not in P
    x = rows(width=128)
    r = blocks.residual_block(P, x, B, NQ, c=torch.zeros((B, PD)))
    assert torch.is_tensor(r) and r is not x and tuple(r.shape) == (B * NQ, 64) and r.dtype == F32
    # fc_q from the fused LN + linear; no packed q | k | v operand at dim_in != dim_out, so the LayerNorm runs once more for the K | V GEMM
    assert names(rec) == ["sgemm", "sgemm", "ln_linear", "layernorm_modulate", "gemm_bf16", "cast_pad_bf16", "gemm_bf16",
                          "attention_oproj_resid_", "ln_mlp_resid_"]
    assert rec.calls[0][1]["w"] is P["wada1"] and rec.calls[1][1]["w"] is P["wada2"]
    assert only(rec, "ln_linear")["w"] is P["wq"] and only(rec, "ln_linear")["mod_sample_stride"] == 2 * 128
    assert only(rec, "layernorm_modulate")["mod_sample_stride"] == 2 * 128 and only(rec, "layernorm_modulate")["rows_per_sample"] == NQ
    assert rec.calls[4][1]["w"] is P["wkv"]
    sc = rec.calls[6][1]
    assert sc["w"] is P["wsc"] and sc["epilogue"] == _lib.EPI_F32
    a = only(rec, "attention_oproj_resid_")
    assert a["x"] is r and a["gate"] is not None and a["gate_sample_stride"] == 4 * 64 and a["Nk"] == NQ
    m = only(rec, "ln_mlp_resid_")
    assert m["x"] is r and (m["mod_sample_stride"], m["rows_per_sample"]) == (4 * 64, NQ)


@pytest.mark.parametrize("norm", ["group_norm", None])
def test_other_norms_take_the_chain_around_the_fused_attention(rec, norm):
    P = pack(rec, dim_c=PD, norm=norm)
    blocks.residual_block(P, rows(), B, NQ, c=torch.zeros((B, PD)))
    norm_kernels = ["group_stats", "norm_apply"] if norm else ["norm_apply"]
    assert names(rec) == ["sgemm"] + norm_kernels + ["gemm_bf16", "gemm_bf16", "attention_oproj_resid_"] + norm_kernels + ["gemm_bf16", "gemm_bf16"]
    gemms = [kw for n, kw in rec.calls if n == "gemm_bf16"]
    assert [g["w"] is w for g, w in zip(gemms, (P["wq"], P["wkv"], P["wup"], P["wdn"]))] == [True] * 4
    assert gemms[1]["x"] is gemms[0]["x"]                                  # self-attention: K | V from the normalised rows
    assert gemms[2]["epilogue"] == _lib.EPI_GELU_BF16 and gemms[3]["epilogue"] == _lib.EPI_RESID_F32 and gemms[3]["gate"] is not None
    for kw in (kw for n, kw in rec.calls if n == "norm_apply"):
        assert kw["shift"] is not None and (kw["mod_sample_stride"], kw["rows_per_sample"], kw["rows_per_stat"]) == (6 * C, NQ, NQ)
        assert (kw["stats"] is not None) == (norm is not None) and (kw["w"] is not None) == (norm is not None)
    if norm:
        assert [kw["groups"] for n, kw in rec.calls if n == "group_stats"] == [16, 16]


def test_decoder_act_takes_the_chain_behind_both_norms(rec):
    P = pack(rec, act="silu")
    assert P["act"] > 0
    blocks.residual_block(P, rows(), B, NQ, kv_pre=torch.zeros((B * NK, 2 * C), dtype=BF), Nk=NK)
    # the fused LN kernels have no activation slot; the attention kernel does not see the norms and stays
    assert names(rec) == ["layernorm_modulate", "block_activation_", "gemm_bf16", "attention_oproj_resid_",
                          "layernorm_modulate", "block_activation_", "gemm_bf16", "gemm_bf16"]
    lns = [kw for n, kw in rec.calls if n == "layernorm_modulate"]
    assert lns[0]["w"] is P["n1"][0] and lns[1]["w"] is P["n2"][0] and lns[0]["shift"] is None
    acts = [kw for n, kw in rec.calls if n == "block_activation_"]
    assert [a["kind"] for a in acts] == [P["act"]] * 2 and acts[0]["x"] is rec.calls[2][1]["x"] and acts[1]["x"] is rec.calls[6][1]["x"]


def test_width_192_with_6_heads_is_the_whole_chain(rec):
    P = pack(rec, C=192, H=6)
    x, xb = rows(width=192), torch.zeros((B * NQ, 192), dtype=BF)
    r = blocks.residual_block_handoff(P, x, B, NQ, NK, torch.zeros((B * NK, 2 * 192), dtype=BF), next_P=P, x_bf16_out=xb,
                                      q_pre=torch.zeros((B * NQ, 192), dtype=BF))
    assert r[0] is x and r[1] is None                                     # no fused MLP kernel at this width: nothing to hand over
    assert names(rec) == ["layernorm_modulate", "gemm_bf16", "attention_fwd", "gemm_bf16",
                          "layernorm_modulate", "gemm_bf16", "gemm_bf16", "cast_pad_bf16"]
    assert rec.calls[1][1]["w"] is P["wq"]                                 # (the chain forms q itself: q_pre is not read)
    assert only(rec, "attention_fwd")["head_dim"] == 32 and only(rec, "attention_fwd")["H"] == 6
    assert only(rec, "cast_pad_bf16")["src"] is x and only(rec, "cast_pad_bf16")["cols_pad"] == 192


def test_row_stride_not_a_multiple_of_4_takes_the_chain(rec):
    P = pack(rec)
    x = torch.zeros((B * NQ, C + 1), dtype=F32)[:, :C]
    assert x.stride(0) % 4 == 1
    assert blocks.residual_block(P, x, B, NQ, y_bf16=torch.zeros((B * NK, C), dtype=BF), Nk=NK) is x
    # both fused LN kernels read rows as float4; the attention kernel takes any row stride of x
    assert names(rec) == ["layernorm_modulate", "gemm_bf16", "gemm_bf16", "attention_oproj_resid_", "layernorm_modulate", "gemm_bf16", "gemm_bf16"]


def test_only_the_handoff_entry_takes_next_p_and_q_pre():
    plain = inspect.signature(blocks.residual_block).parameters
    assert list(plain) == ["P", "x", "B", "Nq", "y_bf16", "Nk", "c", "per_token", "x_bf16_out", "kv_pre"]
    hand = inspect.signature(blocks.residual_block_handoff).parameters
    assert {"kv_pre", "q_pre", "next_P"} <= set(hand)
    assert not hasattr(blocks, "FUSED_MLP") and not hasattr(blocks, "FUSED_ATTN")
