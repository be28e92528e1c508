"""GPU (-m gpu): the attention backward on a long key axis alone, per element (ldt_attention_bwd_wide: csrc/attention_bwd.hip, head width 32,
up to 512 queries on up to 8192 keys; row statistics and dQ formed per chunk of 256 keys and combined in chunk order, dK / dV by the
key-block kernel of ldt_attention_bwd_cross).  Shapes, references and bounds: tests/topdown_train_checks.py (held without a GPU, planted
faults included, by test_topdown_train_host.py).

  * dQ, dK and dV per element against kernel_checks.attn_bwd_ref at head width 32 plus the chunk terms on all three bounds
  * a case in which a whole chunk's exp(m_c - M) underflows
  * where ldt_attention_bwd_cross admits the shape (Nk <= 512): at one chunk dQ, dK, dV and the row statistics bit-equal to its own; at
    more chunks D bit-equal and L within the extra roundings
  * the scratch holds what the header states (each chunk's maximum and sum, then each chunk's unscaled dQ partial), every float of it is
    written, nothing past it; a scratch one float short is refused
  * strided operands inside guard bands stay intact
  * the refusals and their messages
  * a second call repeats bit for bit

Before ldt_attention_bwd_wide existed every test here ended at the missing `ops.attention_bwd_wide`."""
import pytest
import torch

import kernel_checks as kc
import narrow_bwd_checks as nb
import topdown_train_checks as tc

pytestmark = pytest.mark.gpu
DH = 32


def operands(B, H, Nq, Nk, case=None):
    """-> (q, kv, dO on the CPU; q, k, v, o, dO on the device), o the forward kernel's saved output."""
    from ldt_amd import ops
    C = H * DH
    q, kv, do = tc.wide_case(B, H, Nq, Nk) if case is None else case
    q_d, kv_d, do_d = q.cuda(), kv.cuda(), do.cuda()
    k, v = kv_d[:, :C], kv_d[:, C:]
    o = ops.attention_fwd(q_d, k, v, B, H, Nq, Nk, DH)
    return q, kv, do, q_d, k, v, o, do_d


def cross_with_stats(q_d, k, v, o, do_d, B, H, Nq, Nk):
    from ldt_amd import ops
    st = torch.full((B, H, Nq, 2), float("nan"), dtype=torch.float32, device="cuda")
    C = H * DH
    out = ops._attention_bwd("attention_bwd_cross", "ldt_attention_bwd_cross", q_d, k, v, o, do_d, B, H, (Nq, Nk), DH,
                             lambda Cc: (torch.empty((B * Nq, C), dtype=torch.bfloat16, device="cuda"),)
                             + torch.empty((B * Nk, 2 * Cc), dtype=torch.bfloat16, device="cuda").split(Cc, 1), stats_out=st)
    return out, st


@pytest.mark.parametrize("B,H,Nq,Nk", tc.WIDE_SHAPES)
def test_attention_bwd_wide_per_element(B, H, Nq, Nk):
    from ldt_amd import ops
    q, kv, do, q_d, k, v, o, do_d = operands(B, H, Nq, Nk)
    st = torch.full((B, H, Nq, 2), float("nan"), dtype=torch.float32, device="cuda")
    dq, dk, dv = ops.attention_bwd_wide(q_d, k, v, o, do_d, B, H, Nq, Nk, stats_out=st)
    assert tuple(dq.shape) == (B * Nq, H * DH) and tuple(dk.shape) == tuple(dv.shape) == (B * Nk, H * DH)
    assert dk.data_ptr() + 2 * H * DH == dv.data_ptr() and dk.stride(0) == dv.stride(0) == 2 * H * DH       # the halves of one [B Nk, 2 C] tensor
    r = tc.wide_check({"dq": dq, "dk": dk, "dv": dv}, q, kv, o, do, B, H, Nq, Nk, "attention_bwd_wide B%d H%d Nq%d Nk%d" % (B, H, Nq, Nk))
    chunks = -(-Nk // tc.CHUNK)
    print("train-kernel attention_bwd_wide B%d H%d Nq%d Nk%d (%d chunks)  max err/tol dq %.3f dk %.3f dv %.3f" % (B, H, Nq, Nk, chunks, r["dq"], r["dk"], r["dv"]))
    st2 = torch.full_like(st, float("nan"))
    dq2, dk2, dv2 = ops.attention_bwd_wide(q_d, k, v, o, do_d, B, H, Nq, Nk, stats_out=st2)
    assert torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv) and torch.equal(st2, st)     # fixed order: the same bits
    assert bool(st.isfinite().all())
    L64 = torch.logsumexp(nb.scores64(q, kv, B, H, Nq, Nk, DH), -1)
    kc.assert_elementwise(st[..., 0].cpu(), L64, tc.lse_err(q, kv, B, H, Nq, Nk, min(Nk, tc.CHUNK), chunks), "L")
    if Nk <= 512:
        (cq, ck, cv), st_c = cross_with_stats(q_d, k, v, o, do_d, B, H, Nq, Nk)
        assert torch.equal(st[..., 1], st_c[..., 1])                                # D: computed as there
        if chunks == 1:                                                             # one chunk: exp(0) = 1, one partial: the same bits everywhere
            assert torch.equal(st, st_c), "L"
            assert torch.equal(cq, dq) and torch.equal(ck, dk) and torch.equal(cv, dv)
            assert torch.equal(cq.view(torch.int16), dq.view(torch.int16)), "a zero's sign"


def test_a_whole_chunk_underflows():
    from ldt_amd import ops
    B, H, Nq, Nk = tc.UNDERFLOW_SHAPE
    q, kv, do, margin = tc.underflow_case()
    assert margin >= 40.0
    q, kv, do, q_d, k, v, o, do_d = operands(B, H, Nq, Nk, (q, kv, do))
    need = ops.attention_bwd_wide_scratch(B, H, Nq, Nk)
    scratch = torch.full((need,), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((B, H, Nq, 2), float("nan"), dtype=torch.float32, device="cuda")
    dq, dk, dv = ops.attention_bwd_wide(q_d, k, v, o, do_d, B, H, Nq, Nk, scratch=scratch, stats_out=st)
    cs = scratch[:3 * B * H * Nq * 2].view(3, B, H, Nq, 2)
    assert bool(((cs[1, ..., 0] - cs[0, ..., 0]) >= 40.0).all()) and bool(((cs[1, ..., 0] - cs[2, ..., 0]) >= 40.0).all())
    assert bool(st.isfinite().all())
    r = tc.wide_check({"dq": dq, "dk": dk, "dv": dv}, q, kv, o, do, B, H, Nq, Nk, "underflowing chunk")
    print("train-kernel attention_bwd_wide underflowing chunk  max err/tol dq %.3f dk %.3f dv %.3f" % (r["dq"], r["dk"], r["dv"]))
    (cq, ck, cv), st_c = cross_with_stats(q_d, k[CH_LO:CH_HI], v[CH_LO:CH_HI], o, do_d, B, H, Nq, CH_HI - CH_LO)
    # chunk 1 alone decides L (the other chunks' terms vanish beside its sum in fp32): the statistics of that chunk's keys alone, bit for bit
    assert torch.equal(st_c[..., 0], st[..., 0])


CH_LO, CH_HI = tc.CHUNK, 2 * tc.CHUNK            # the live chunk's keys (B = 1: rows of the one sample)


@pytest.mark.parametrize("B,H,Nq,Nk", [(2, 2, 32, 296), (1, 4, 72, 552)])
def test_scratch_layout_and_length(B, H, Nq, Nk):
    """The two regions hold what the header states; every float of them is written and none past them; one float short is refused."""
    from ldt_amd import ops
    from ldt_amd._lib import LdtHipError
    C = H * DH
    q, kv, do, q_d, k, v, o, do_d = operands(B, H, Nq, Nk)
    chunks, need = -(-Nk // tc.CHUNK), ops.attention_bwd_wide_scratch(B, H, Nq, Nk)
    assert need == chunks * B * H * Nq * 2 + chunks * B * Nq * C
    scratch = torch.full((need + 4096,), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((B, H, Nq, 2), float("nan"), dtype=torch.float32, device="cuda")
    dq, dk, dv = ops.attention_bwd_wide(q_d, k, v, o, do_d, B, H, Nq, Nk, scratch=scratch, stats_out=st)
    assert bool(scratch[need:].isnan().all()) and bool(scratch[:need].isfinite().all())
    cs = scratch[:chunks * B * H * Nq * 2].view(chunks, B, H, Nq, 2).cpu()
    parts = scratch[chunks * B * H * Nq * 2:need].view(chunks, B, Nq, C)
    s64 = nb.scores64(q, kv, B, H, Nq, Nk, DH)
    e_s = tc.score_err(q, kv, B, H, Nq, Nk)
    for c in range(chunks):
        sl = s64[..., c * tc.CHUNK:min((c + 1) * tc.CHUNK, Nk)]
        m64 = sl.max(-1).values
        kc.assert_elementwise(cs[c, ..., 0], m64, e_s, "chunk %d maximum" % c)
        sum64 = torch.exp(sl - m64[..., None]).sum(-1)
        kc.assert_elementwise(cs[c, ..., 1], sum64, sum64 * (2 * e_s + (sl.shape[-1] // 16 + 6) * kc.U24 + kc.LIBM_ABS), "chunk %d sum" % c)
    M = cs[..., 0].max(0).values                                                    # the combination, restated on the device's own pairs
    tot = torch.zeros_like(M)
    for c in range(chunks):
        tot = tot + cs[c, ..., 1] * torch.exp(cs[c, ..., 0] - M)
    kc.assert_elementwise(st[..., 0].cpu(), (M.double() + torch.log(tot.double())), ((chunks + 3) * kc.U24 + kc.LIBM_ABS) + 2 * kc.U24 * M.abs().double(), "L from the pairs")
    sc = float(torch.tensor(1.0) / torch.tensor(float(DH)).sqrt())                   # the entry point's 1.0f / sqrtf(32.f)
    tot = torch.zeros_like(parts[0])
    for c in range(chunks):
        tot = tot + parts[c]
    assert torch.equal(dq, (tot * sc).to(torch.bfloat16).view(B * Nq, C))           # added in chunk order, scaled once, rounded once
    with pytest.raises(LdtHipError, match=r"ldt_attention_bwd_wide failed \(status -1\): attention_bwd_wide: scratch holds %d floats" % (need - 1)):
        ops.attention_bwd_wide(q_d, k, v, o, do_d, B, H, Nq, Nk, scratch=scratch[:need - 1])
    dq2, _, _ = ops.attention_bwd_wide(q_d, k, v, o, do_d, B, H, Nq, Nk, scratch=scratch[:need])
    assert torch.equal(dq2, dq)


def test_outputs_as_interiors_of_guarded_buffers():
    """dQ and dK | dV as interiors of sentinel-filled buffers whose strides exceed their widths, q and K | V as column blocks of buffers
    whose spare columns are NaN: bit-equal to the dense call, the surround intact bit for bit."""
    from ldt_amd import ops
    B, H, Nq, Nk = 2, 2, 24, 296
    C = H * DH
    _, _, _, q, k, v, o, do_d = operands(B, H, Nq, Nk)
    dq0, dk0, dv0 = ops.attention_bwd_wide(q, k, v, o, do_d, B, H, Nq, Nk)
    wq = torch.full((B * Nq, C + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    wkv = torch.full((B * Nk, 2 * C + 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    wq[:, :C], wkv[:, :C], wkv[:, C + 8:2 * C + 8] = q, k, v
    big_q = torch.full((B * Nq + 2, C + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    big_kv = torch.full((B * Nk + 3, 2 * C + 40), float("nan"), dtype=torch.bfloat16, device="cuda")
    dq_out, dkv_out = big_q[1:B * Nq + 1, 8:C + 8], big_kv[2:B * Nk + 2, 16:2 * C + 16]
    dq, dk, dv = ops.attention_bwd_wide(wq[:, :C], wkv[:, :C], wkv[:, C + 8:2 * C + 8], o, do_d, B, H, Nq, Nk, dq_out=dq_out, dkv_out=dkv_out)
    assert dq.data_ptr() == dq_out.data_ptr() and dk.data_ptr() == dkv_out.data_ptr()
    assert torch.equal(dq_out, dq0) and torch.equal(dkv_out, torch.cat([dk0, dv0], 1))
    keep = torch.ones_like(big_q, dtype=torch.bool)
    keep[1:B * Nq + 1, 8:C + 8] = False
    assert bool((big_q[keep] == 7).all())
    keep = torch.ones_like(big_kv, dtype=torch.bool)
    keep[2:B * Nk + 2, 16:2 * C + 16] = False
    assert bool(big_kv[keep].isnan().all()) and not bool(dkv_out.isnan().any())
    assert bool(wq[:, C:].isnan().all()) and bool(wkv[:, C:C + 8].isnan().all()) and bool(wkv[:, 2 * C + 8:].isnan().all())


def test_refusals_leave_the_device_idle():
    from ldt_amd import _lib, ops
    from ldt_amd._lib import LdtHipError
    assert (_lib.ATTN_BWD_WIDE_MAX_QUERIES, _lib.ATTN_BWD_WIDE_MAX_KEYS) == (512, 8192)
    B, H = 1, 2
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    kv = z(8, 4 * 64)
    with pytest.raises(LdtHipError, match=r"ldt_attention_bwd_wide failed \(status -2\): attention_bwd_wide: head_dim 64 \(32 only\)"):
        ops.attention_bwd_wide(z(8, 128), kv[:, :128], kv[:, 128:], z(B, H, 8, 64), z(B, H, 8, 64), B, H, 8, 8, head_dim=64)
    C = H * DH
    for Nq, Nk in ((8, 8200), (520, 8)):
        kv = z(B * Nk, 2 * C)
        with pytest.raises(LdtHipError, match=r"ldt_attention_bwd_wide failed \(status -2\): attention_bwd_wide: Nq %d, Nk %d \(1 <= Nq <= 512, 1 <= Nk <= 8192\)" % (Nq, Nk)):
            ops.attention_bwd_wide(z(B * Nq, C), kv[:, :C], kv[:, C:], z(B, H, Nq, DH), z(B, H, Nq, DH), B, H, Nq, Nk)
    kv = z(B * 8, 2 * C)
    with pytest.raises(LdtHipError, match="scratch holds 100 floats"):
        ops.attention_bwd_wide(z(B * 8, C), kv[:, :C], kv[:, C:], z(B, H, 8, DH), z(B, H, 8, DH), B, H, 8, 8,
                               scratch=torch.zeros(100, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="q .* for B 1, Nq 8, Nk 16"):
        ops.attention_bwd_wide(z(B * 8, C), kv[:, :C], kv[:, C:], z(B, H, 8, DH), z(B, H, 8, DH), B, H, 8, 16)      # 8 key rows where 16 are announced
    torch.cuda.synchronize()
    # ldt_attention_bwd_cross keeps its own limits
    kv = z(B * 520, 2 * C)
    with pytest.raises(LdtHipError, match="attention_bwd_cross: .*Nq 8, Nk 520"):
        ops.attention_bwd_cross(z(B * 8, C), kv[:, :C], kv[:, C:], z(B, H, 8, DH), z(B, H, 8, DH), B, H, 8, 520, DH)
