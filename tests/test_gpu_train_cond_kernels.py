"""GPU (-m gpu): the cross-attention backward alone, per element (ldt_attention_bwd_cross: csrc/attention_bwd.hip, the MFMA form at
head widths 32 and 64, the narrow form at 8 and 16, with Nq query rows and Nk key rows).  Shapes and operands: tests/cross_bwd_checks.py;
the bound: kernel_checks.attn_bwd_ref with the two lengths apart (test_train_cond_host.py holds it without a GPU, planted faults included).

  * every output element against float64 from the very bf16 operands, inside the componentwise bound; two launches bit-equal
  * at Nq = Nk the same bits as ops.attention_bwd, at all four head widths
  * an exact probe on dV: one-hot attention by construction, dV = the selecting query's dO row, unselected keys exactly 0
  * dQ and dK | dV written into the interiors of sentinel-surrounded buffers with wider strides: values equal, surround intact
  * argument errors leave the device idle

Before ldt_attention_bwd_cross existed every test here ended at the missing `ops.attention_bwd_cross`."""
import pytest
import torch

import cross_bwd_checks as cb
import narrow_bwd_checks as nb

pytestmark = pytest.mark.gpu


def operands(B, H, Nq, Nk, Dh, large=False, seed=None):
    """-> (q, kv, dO on the CPU; q, k, v, o, dO on the device), o the forward kernel's saved output."""
    from ldt_amd import ops
    C = H * Dh
    q, kv, do = cb.cross_case(B, H, Nq, Nk, Dh, large, seed)
    q_d, kv_d, do_d = q.cuda(), kv.cuda(), do.cuda()
    k, v = kv_d[:, :C], kv_d[:, C:]
    o = ops.attention_fwd(q_d, k, v, B, H, Nq, Nk, Dh)
    return q, kv, do, q_d, k, v, o, do_d


@pytest.mark.parametrize("B,H,Nq,Nk,Dh,large", cb.CASES)
def test_attention_bwd_cross_per_element(B, H, Nq, Nk, Dh, large):
    from ldt_amd import ops
    q, kv, do, q_d, k, v, o, do_d = operands(B, H, Nq, Nk, Dh, large)
    if large:
        s = nb.scores64(q, kv, B, H, Nq, Nk, Dh)
        assert float(s.amax(-1).min()) > 25 and float(s.amax(-1).max()) > 89       # past fp32 exp's range
    dq, dk, dv = ops.attention_bwd_cross(q_d, k, v, o, do_d, B, H, Nq, Nk, Dh)
    assert tuple(dq.shape) == (B * Nq, H * Dh) and tuple(dk.shape) == tuple(dv.shape) == (B * Nk, H * Dh)
    assert dk.data_ptr() + 2 * H * Dh == dv.data_ptr() and dk.stride(0) == dv.stride(0) == 2 * H * Dh       # the halves of one [B Nk, 2 C] tensor
    r = nb.check({"dq": dq, "dk": dk, "dv": dv}, q, kv, o, do, B, H, Nq, Nk, Dh,
                 "attention_bwd_cross B%d H%d Nq%d Nk%d Dh%d large=%d" % (B, H, Nq, Nk, Dh, large))
    print("train-kernel attention_bwd_cross B%d H%d Nq%d Nk%d Dh%d large=%d (P, dS %s)  max err/tol %.3f"
          % (B, H, Nq, Nk, Dh, large, "bf16" if nb.rounds(Dh) else "fp32", r))
    dq2, dk2, dv2 = ops.attention_bwd_cross(q_d, k, v, o, do_d, B, H, Nq, Nk, Dh)
    assert torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv)  # fixed order: the same bits


@pytest.mark.parametrize("B,H,N,Dh", cb.SQUARE)
def test_square_problem_equals_the_self_attention_entry_points(B, H, N, Dh):
    from ldt_amd import ops
    C = H * Dh
    qkv, do = nb.attn_case(B, H, N, Dh)
    qkv_d, do_d = qkv.cuda(), do.cuda()
    q, k, v = qkv_d[:, :C], qkv_d[:, C:2 * C], qkv_d[:, 2 * C:]
    o = ops.attention_fwd(q, k, v, B, H, N, N, Dh)
    want = ops.attention_bwd(q, k, v, o, do_d, B, H, N, head_dim=Dh)
    got = ops.attention_bwd_cross(q, k, v, o, do_d, B, H, N, N, Dh)
    for nm, a, b in zip(("dq", "dk", "dv"), got, want):
        assert torch.equal(a, b), nm


@pytest.mark.parametrize("B,H,Nq,Nk,Dh", cb.PROBES)
def test_exact_selection_probe_on_dv(B, H, Nq, Nk, Dh):
    """One-hot attention by construction (cross_bwd_checks.selection_probe): dV[pi(i)] = dO[i] bit for bit, unselected keys exactly 0.
    A key loop that stopped at Nq, a query loop that stopped at Nk, statistics read at the other length's stride or a dO row taken
    from the wrong query all move or lose a row."""
    from ldt_amd import ops
    C = H * Dh
    q, kv, do, pi, lead = cb.selection_probe(B, H, Nq, Nk, Dh, seed=31 + Nq + Nk + Dh)
    s = nb.scores64(q, kv, B, H, Nq, Nk, Dh)
    top2 = s.topk(min(2, Nk), -1).values
    assert torch.equal(s.argmax(-1), pi) and (Nk == 1 or float((top2[..., 0] - top2[..., 1]).min()) >= 110)
    q_d, kv_d, do_d = q.cuda(), kv.cuda(), do.cuda()
    k, v = kv_d[:, :C], kv_d[:, C:]
    o = ops.attention_fwd(q_d, k, v, B, H, Nq, Nk, Dh)
    _, _, dv = ops.attention_bwd_cross(q_d, k, v, o, do_d, B, H, Nq, Nk, Dh)
    want = cb.selection_expected_dv(do, pi, B, H, Nq, Nk, Dh)
    assert torch.equal(dv.cpu(), want)
    if Nq < Nk:
        assert bool((want.view(B, Nk, H, Dh).abs().sum(-1) == 0).any())            # there are unselected keys, and they are exactly 0


@pytest.mark.parametrize("B,H,Nq,Nk,Dh", [(2, 2, 8, 24, 64), (1, 1, 40, 72, 32), (2, 3, 33, 17, 16), (1, 2, 17, 33, 8)])
def test_outputs_as_interiors_of_guarded_buffers(B, H, Nq, Nk, Dh):
    """dQ and dK | dV as interiors of sentinel-filled buffers whose strides exceed their widths, q and K | V as column blocks of buffers
    whose spare columns are NaN: bit-equal to the dense call, the surround intact bit for bit."""
    from ldt_amd import ops
    C = H * Dh
    _, _, _, q, k, v, o, do_d = operands(B, H, Nq, Nk, Dh)
    dq0, dk0, dv0 = ops.attention_bwd_cross(q, k, v, o, do_d, B, H, Nq, Nk, Dh)
    wq = torch.full((B * Nq, C + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    wkv = torch.full((B * Nk, 2 * C + 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    wq[:, :C], wkv[:, :C], wkv[:, C + 8:2 * C + 8] = q, k, v
    big_q = torch.full((B * Nq + 2, C + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    big_kv = torch.full((B * Nk + 3, 2 * C + 40), float("nan"), dtype=torch.bfloat16, device="cuda")
    dq_out, dkv_out = big_q[1:B * Nq + 1, 8:C + 8], big_kv[2:B * Nk + 2, 16:2 * C + 16]
    dq, dk, dv = ops.attention_bwd_cross(wq[:, :C], wkv[:, :C], wkv[:, C + 8:2 * C + 8], o, do_d, B, H, Nq, Nk, Dh, dq_out=dq_out, dkv_out=dkv_out)
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
    from ldt_amd import ops
    from ldt_amd._lib import LdtHipError
    B, H, Dh = 1, 2, 8
    C = H * Dh
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="head_dim 24 is not 8, 16, 32 or 64"):
        ops.attention_bwd_cross(z(8, 48), z(8, 48), z(8, 48), z(B, H, 8, 24), z(B, H, 8, 24), B, H, 8, 8, 24)
    for Nq, Nk in ((520, 8), (8, 520)):
        kv = z(B * Nk, 2 * C)
        with pytest.raises(LdtHipError, match=r"ldt_attention_bwd_cross failed \(status -2\): attention_bwd_cross: .*Nq %d, Nk %d" % (Nq, Nk)):
            ops.attention_bwd_cross(z(B * Nq, C), kv[:, :C], kv[:, C:], z(B, H, Nq, Dh), z(B, H, Nq, Dh), B, H, Nq, Nk, Dh)
    with pytest.raises(ValueError, match="q .* for B 1, Nq 8, Nk 16"):
        kv = z(B * 8, 2 * C)                                                       # 8 key rows where 16 are announced
        ops.attention_bwd_cross(z(B * 8, C), kv[:, :C], kv[:, C:], z(B, H, 8, Dh), z(B, H, 8, Dh), B, H, 8, 16, Dh)
    torch.cuda.synchronize()
