"""GPU (-m gpu): the attention backward at head widths 8, 16 and 32 alone, per element (ldt_attention_bwd_narrow: csrc/attention_bwd.hip, the
narrow form for 8 and 16, the MFMA form instantiated at 32).  Helpers and shapes: tests/narrow_bwd_checks.py; the bound:
kernel_checks.attn_bwd_ref (validated without a GPU, planted faults included, by test_train_narrow_host.py).

Every case is compared with float64 computed from the very bf16 inputs the kernel read (O from ops.attention_fwd, as training keeps it), with
kernel_checks.assert_elementwise: err / tol <= 1 for every element of dq, dk and dv.  Then the layout: a second call gives the same bits, a
one-hot dO row stays in its head (quirk Q1), strided operands in NaN-surrounded buffers give the dense result and leave the surround alone,
and bad arguments are refused before anything is launched.  Each test prints its largest err / tol (-s); DESIGN.md section 4.13 records them.
Before ldt_attention_bwd_narrow existed every test here ended in ldt_attention_bwd's "64 only"."""
import pytest
import torch

import narrow_bwd_checks as nb

pytestmark = pytest.mark.gpu


def operands(B, H, N, Dh, large=False, seed=None):
    from ldt_amd import ops
    C = H * Dh
    qkv, do = nb.attn_case(B, H, N, Dh, large, seed)
    qkv_d, do_d = qkv.cuda(), do.cuda()
    q, k, v = qkv_d[:, :C], qkv_d[:, C:2 * C], qkv_d[:, 2 * C:]
    return qkv, do, q, k, v, ops.attention_fwd(q, k, v, B, H, N, N, Dh), do_d     # o: the saved forward output, as training keeps it


@pytest.mark.parametrize("B,H,N,Dh,large", nb.CASES)
def test_attention_bwd_narrow_per_element(B, H, N, Dh, large):
    from ldt_amd import ops
    qkv, do, q, k, v, o, do_d = operands(B, H, N, Dh, large)
    if large:
        s = nb.scores64(*nb.split(qkv), B, H, N, N, Dh)
        assert float(s.amax(-1).min()) > 25 and float(s.amax(-1).max()) > 89      # a backward without the recomputed maximum overflows
    dq, dk, dv = ops.attention_bwd(q, k, v, o, do_d, B, H, N, head_dim=Dh)
    assert dq.shape == dk.shape == dv.shape == (B * N, H * Dh) and dq.dtype == torch.bfloat16
    r = nb.check({"dq": dq, "dk": dk, "dv": dv}, *nb.split(qkv), o, do, B, H, N, N, Dh, "attention_bwd B%d H%d N%d Dh%d large=%d" % (B, H, N, Dh, large))
    print("train-kernel attention_bwd B%d H%d N%d Dh%d large=%d (P, dS %s)  max err/tol %.3f" % (B, H, N, Dh, large, "bf16" if nb.rounds(Dh) else "fp32", r))
    dq2, dk2, dv2 = ops.attention_bwd(q, k, v, o, do_d, B, H, N, head_dim=Dh)
    assert torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv)     # fixed order: the same bits


@pytest.mark.parametrize("B,H,N,Dh", [(2, 4, 8, 8), (2, 2, 8, 16)])
def test_attention_bwd_narrow_q1_probe(B, H, N, Dh):
    """Quirk Q1: dO is the raw [B][H][N][Dh] buffer.  A gradient in the single row [b][h][n] reaches dV and dK only in head h of sample b and
    dQ only in row n: exact zeros elsewhere.  A kernel that read dO as (B, N, H, Dh) rows would spread it over other heads or tokens."""
    from ldt_amd import ops
    _, _, q, k, v, o, _ = operands(B, H, N, Dh, seed=5)
    for b, h, n in ((1, 0, 5), (0, H - 1, 2)):
        do = torch.zeros(B, H, N, Dh, dtype=torch.bfloat16, device="cuda")
        do[b, h, n] = 1.0
        dq, dk, dv = ops.attention_bwd(q, k, v, o, do, B, H, N, head_dim=Dh)
        inside = torch.zeros(B, N, H, Dh, dtype=torch.bool, device="cuda")
        inside[b, :, h] = True
        dv4, dq4, dk4 = dv.reshape(B, N, H, Dh), dq.reshape(B, N, H, Dh), dk.reshape(B, N, H, Dh)
        assert float(dv4[~inside].abs().max()) == 0.0 and bool((dv4[inside] != 0).all())
        assert float(dk4[~inside].abs().max()) == 0.0 and float(dk4[inside].abs().max()) > 0.0
        only_row = torch.zeros_like(inside)
        only_row[b, n, h] = True
        assert float(dq4[~only_row].abs().max()) == 0.0 and float(dq4[only_row].abs().max()) > 0.0


@pytest.mark.parametrize("B,H,N,Dh", [(2, 3, 8, 8), (1, 2, 72, 16), (2, 4, 33, 32)])
def test_attention_bwd_narrow_strided_operands(B, H, N, Dh):
    """q, k, v as column blocks of a [B N, 3 C + 8] buffer whose spare columns are NaN, `out` a view of a wider sentinel buffer: bit-equal to
    the dense call, the surround intact bit for bit."""
    from ldt_amd import ops
    C = H * Dh
    _, _, q, k, v, o, do_d = operands(B, H, N, Dh)
    dense = torch.cat(ops.attention_bwd(q, k, v, o, do_d, B, H, N, head_dim=Dh), 1)
    wide = torch.full((B * N, 3 * C + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    wide[:, :C], wide[:, C:2 * C], wide[:, 2 * C:3 * C] = q, k, v
    big = torch.full((B * N + 2, 3 * C + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    out = big[1:B * N + 1, 8:3 * C + 8]
    dq, dk, dv = ops.attention_bwd(wide[:, :C], wide[:, C:2 * C], wide[:, 2 * C:3 * C], o, do_d, B, H, N, head_dim=Dh, out=out)
    assert dq.data_ptr() == out.data_ptr() and torch.equal(out, dense)
    assert torch.equal(torch.cat([dq, dk, dv], 1), dense)
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[1:B * N + 1, 8:3 * C + 8] = False
    assert bool((big[keep] == 7).all())
    assert bool(wide[:, 3 * C:].isnan().all()) and torch.equal(wide[:, :3 * C], torch.cat([q, k, v], 1))


def test_attention_bwd_narrow_refusals_leave_the_device_idle():
    from ldt_amd import ops
    from ldt_amd._lib import LdtHipError
    B, H = 1, 2
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    qkv = z(B * 8, 3 * H * 24)
    with pytest.raises(ValueError, match="head_dim 24 is not 8, 16, 32 or 64"):
        ops.attention_bwd(qkv[:, :48], qkv[:, 48:96], qkv[:, 96:], z(B, H, 8, 24), z(B, H, 8, 24), B, H, 8, head_dim=24)
    N, C = 520, H * 8
    qkv = z(B * N, 3 * C)
    with pytest.raises(LdtHipError, match=r"ldt_attention_bwd_narrow failed \(status -2\): attention_bwd_narrow: .*N 520 \(self-attention, N <= 512\)"):
        ops.attention_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], z(B, H, N, 8), z(B, H, N, 8), B, H, N, head_dim=8)
    torch.cuda.synchronize()
