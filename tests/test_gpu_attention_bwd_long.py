"""GPU (-m gpu): the attention backward on a long query axis alone, per element (ldt_attention_bwd_long: csrc/attention_bwd.hip, head width
32, up to 8192 queries on up to 512 keys; dK / dV summed per chunk of 256 queries into fp32 partials that a second kernel adds in chunk
order).  Shapes, references and bounds: tests/decoder_train_checks.py (held without a GPU, planted faults included, by
test_decoder_train_host.py).

  * dQ, dK and dV per element against kernel_checks.attn_bwd_ref at head width 32, the partial-sum term added to the dK / dV bound
  * where ldt_attention_bwd_cross admits the shape (Nq <= 512): dQ and the row statistics `stats` bit-equal to its own, and at one
    chunk dK / dV too
  * with dO zero outside one chunk, every other chunk's partial of dK and dV in the scratch is exactly 0, and the scratch past the
    partials is never written
  * strided operands inside guard bands stay intact
  * the refusals and their messages: head width 64, Nq = 8200, Nk = 520, a short scratch
  * a second call repeats bit for bit

Before ldt_attention_bwd_long existed every test here ended at the missing `ops.attention_bwd_long`."""
import pytest
import torch

import decoder_train_checks as dc

pytestmark = pytest.mark.gpu
DH = 32


def operands(B, H, Nq, Nk, seed=None):
    """-> (q, kv, dO on the CPU; q, k, v, o, dO on the device), o the forward kernel's saved output."""
    from ldt_amd import ops
    C = H * DH
    q, kv, do = dc.long_case(B, H, Nq, Nk, seed)
    q_d, kv_d, do_d = q.cuda(), kv.cuda(), do.cuda()
    k, v = kv_d[:, :C], kv_d[:, C:]
    o = ops.attention_fwd(q_d, k, v, B, H, Nq, Nk, DH)
    return q, kv, do, q_d, k, v, o, do_d


@pytest.mark.parametrize("B,H,Nq,Nk", dc.LONG_SHAPES)
def test_attention_bwd_long_per_element(B, H, Nq, Nk):
    from ldt_amd import ops
    q, kv, do, q_d, k, v, o, do_d = operands(B, H, Nq, Nk)
    dq, dk, dv = ops.attention_bwd_long(q_d, k, v, o, do_d, B, H, Nq, Nk)
    assert tuple(dq.shape) == (B * Nq, H * DH) and tuple(dk.shape) == tuple(dv.shape) == (B * Nk, H * DH)
    assert dk.data_ptr() + 2 * H * DH == dv.data_ptr() and dk.stride(0) == dv.stride(0) == 2 * H * DH       # the halves of one [B Nk, 2 C] tensor
    r = dc.long_check({"dq": dq, "dk": dk, "dv": dv}, q, kv, o, do, B, H, Nq, Nk, "attention_bwd_long B%d H%d Nq%d Nk%d" % (B, H, Nq, Nk))
    print("train-kernel attention_bwd_long B%d H%d Nq%d Nk%d (%d chunks)  max err/tol dq %.3f dk %.3f dv %.3f"
          % (B, H, Nq, Nk, -(-Nq // dc.CHUNK), r["dq"], r["dk"], r["dv"]))
    dq2, dk2, dv2 = ops.attention_bwd_long(q_d, k, v, o, do_d, B, H, Nq, Nk)
    assert torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv)  # fixed order: the same bits
    if Nq <= 512:
        st_long, st_cross = (torch.full((B, H, Nq, 2), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
        lq, _, _ = ops.attention_bwd_long(q_d, k, v, o, do_d, B, H, Nq, Nk, stats_out=st_long)
        cq, ck, cv = ops.attention_bwd_cross(q_d, k, v, o, do_d, B, H, Nq, Nk, DH)
        # (attention_bwd_cross's parameter list is held by an earlier test: its statistics buffer is reached through the shared body)
        sq, _, _ = ops._attention_bwd("attention_bwd_cross", "ldt_attention_bwd_cross", q_d, k, v, o, do_d, B, H, (Nq, Nk), DH,
                                      lambda Cc: (torch.empty_like(cq),) + torch.empty((B * Nk, 2 * Cc), dtype=torch.bfloat16, device="cuda").split(Cc, 1),
                                      stats_out=st_cross)
        assert torch.equal(sq, cq)
        assert torch.equal(cq, dq) and torch.equal(lq, dq)                          # the same statistics and dQ kernels:
        assert bool(st_long.isfinite().all()) and torch.equal(st_long, st_cross)    # dQ and (L, D) of every query row, bit for bit
        if Nq <= dc.CHUNK:
            assert torch.equal(ck, dk) and torch.equal(cv, dv)                      # one chunk: the same sums in the same order


@pytest.mark.parametrize("B,H,Nq,Nk,live", [(2, 2, 296, 32, 1), (1, 4, 552, 72, 1), (1, 4, 552, 72, 0)])
def test_a_chunk_contributes_only_its_own_queries(B, H, Nq, Nk, live):
    """dO is zero outside chunk `live`: D and dP vanish for every other query, so dS = P (dP - D) and P^T dO are exactly 0 there and every
    other chunk's partial is exactly 0 — a chunk that read another chunk's queries, dO rows or statistics would leave something."""
    from ldt_amd import ops
    C = H * DH
    q, kv, do, q_d, k, v, o, do_d = operands(B, H, Nq, Nk)
    lo, hi = live * dc.CHUNK, min((live + 1) * dc.CHUNK, Nq)
    do_d = do_d.clone()
    do_d[:, :, :lo] = 0
    do_d[:, :, hi:] = 0
    chunks, need = -(-Nq // dc.CHUNK), ops.attention_bwd_long_scratch(B, H, Nq, Nk)
    assert need == chunks * B * Nk * 2 * C
    scratch = torch.full((need + 4096,), float("nan"), dtype=torch.float32, device="cuda")
    dq, dk, dv = ops.attention_bwd_long(q_d, k, v, o, do_d, B, H, Nq, Nk, scratch=scratch)
    parts = scratch[:need].view(chunks, B, Nk, 2 * C)
    assert bool(scratch[need:].isnan().all()) and bool(parts.isfinite().all())      # every partial written, nothing past them
    for c in range(chunks):
        if c != live:
            assert bool((parts[c] == 0).all()), "chunk %d" % c
    assert bool((parts[live] != 0).any())
    sc = float(torch.tensor(1.0) / torch.tensor(float(DH)).sqrt())                  # the entry point's 1.0f / sqrtf(32.f)
    assert torch.equal(dk, (parts[live, ..., :C] * sc).to(torch.bfloat16).view(B * Nk, C))
    assert torch.equal(dv, parts[live, ..., C:].to(torch.bfloat16).reshape(B * Nk, C))
    assert bool((dq.view(B, Nq, C)[:, :lo] == 0).all()) and bool((dq.view(B, Nq, C)[:, hi:] == 0).all())
    dc.long_check({"dq": dq, "dk": dk, "dv": dv}, q, kv, o, do_d.cpu(), B, H, Nq, Nk, "one live chunk")


@pytest.mark.parametrize("B,H,Nq,Nk", [(2, 2, 296, 32), (1, 1, 40, 72)])
def test_outputs_as_interiors_of_guarded_buffers(B, H, Nq, Nk):
    """dQ and dK | dV as interiors of sentinel-filled buffers whose strides exceed their widths, q and K | V as column blocks of buffers
    whose spare columns are NaN: bit-equal to the dense call, the surround intact bit for bit."""
    from ldt_amd import ops
    C = H * DH
    _, _, _, q, k, v, o, do_d = operands(B, H, Nq, Nk)
    dq0, dk0, dv0 = ops.attention_bwd_long(q, k, v, o, do_d, B, H, Nq, Nk)
    wq = torch.full((B * Nq, C + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    wkv = torch.full((B * Nk, 2 * C + 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    wq[:, :C], wkv[:, :C], wkv[:, C + 8:2 * C + 8] = q, k, v
    big_q = torch.full((B * Nq + 2, C + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    big_kv = torch.full((B * Nk + 3, 2 * C + 40), float("nan"), dtype=torch.bfloat16, device="cuda")
    dq_out, dkv_out = big_q[1:B * Nq + 1, 8:C + 8], big_kv[2:B * Nk + 2, 16:2 * C + 16]
    dq, dk, dv = ops.attention_bwd_long(wq[:, :C], wkv[:, :C], wkv[:, C + 8:2 * C + 8], o, do_d, B, H, Nq, Nk, dq_out=dq_out, dkv_out=dkv_out)
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
    assert (_lib.ATTN_BWD_LONG_MAX_QUERIES, _lib.ATTN_BWD_LONG_MAX_KEYS) == (8192, 512)
    B, H = 1, 2
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    kv = z(8, 4 * 64)
    with pytest.raises(LdtHipError, match=r"ldt_attention_bwd_long failed \(status -2\): attention_bwd_long: head_dim 64 \(32 only\)"):
        ops.attention_bwd_long(z(8, 128), kv[:, :128], kv[:, 128:], z(B, H, 8, 64), z(B, H, 8, 64), B, H, 8, 8, head_dim=64)
    C = H * DH
    for Nq, Nk in ((8200, 8), (8, 520)):
        kv = z(B * Nk, 2 * C)
        with pytest.raises(LdtHipError, match=r"ldt_attention_bwd_long failed \(status -2\): attention_bwd_long: Nq %d, Nk %d \(1 <= Nq <= 8192, 1 <= Nk <= 512\)" % (Nq, Nk)):
            ops.attention_bwd_long(z(B * Nq, C), kv[:, :C], kv[:, C:], z(B, H, Nq, DH), z(B, H, Nq, DH), B, H, Nq, Nk)
    kv = z(B * 8, 2 * C)
    with pytest.raises(LdtHipError, match="scratch holds 100 floats"):
        ops.attention_bwd_long(z(B * 8, C), kv[:, :C], kv[:, C:], z(B, H, 8, DH), z(B, H, 8, DH), B, H, 8, 8,
                               scratch=torch.zeros(100, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="q .* for B 1, Nq 8, Nk 16"):
        ops.attention_bwd_long(z(B * 8, C), kv[:, :C], kv[:, C:], z(B, H, 8, DH), z(B, H, 8, DH), B, H, 8, 16)      # 8 key rows where 16 are announced
    torch.cuda.synchronize()
    # ldt_attention_bwd_cross keeps its own limits
    kv = z(B * 8, 2 * C)
    with pytest.raises(LdtHipError, match="attention_bwd_cross: .*Nq 520, Nk 8"):
        ops.attention_bwd_cross(z(B * 520, C), kv[:, :C], kv[:, C:], z(B, H, 520, DH), z(B, H, 520, DH), B, H, 520, 8, DH)
