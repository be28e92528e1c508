"""GPU (-m gpu): the C++ Score forward (`ldt_score_forward`, csrc/api.hip score_forward_impl, unfolded branch) held stage by stage
(tests/infer_tape.py audit_score_stages; its teeth are shown on the CPU by test_infer_tape_host.py).

The goldens hold a whole forward at 1e-4 and the stand-alone tests every kernel on operands the test built.  Inside the forward QKV, Ob, U,
Hb and X are reused across blocks and the AdaLN rows are addressed as m + k D into one table: a stale buffer or an offset off by one block
moves the result by one residual increment.  No proxy sees the launches, but the workspace is `Score._workspace`'s, the plan a struct
`Score.plan` fills and the table a tensor of the caller's: plans cut to their first n blocks and tables with a gate zeroed leave every stage's
input and output in the workspace.  Each stage is then held from device-observed inputs only, with the bound that holds its kernel alone.
What this rests on is asserted first: two runs of a prefix leave the same bits, what is observed is finite (the workspace is filled with NaN
before every run), a zeroed gate_mlp leaves that block's Ob and U alone, the unedited plan's eps_out is the prefix-L run's, and, once per
GEMM route, a residual GEMM under a zero gate returns its residual operand.  The LN-folded plans are outside (`fold` is asserted absent).
The worst err / bound per stage is printed (-s); DESIGN.md section 4.20 records them."""
import pytest
import torch

import infer_tape as it
import train_tape as tt

pytestmark = pytest.mark.gpu

WORST = {}
# name: hidden, heads, blocks, B, T, cond_tokens, shared table (z = 120, t_dim = 64 throughout)
CASES = {
    "tiny": (128, 2, 2, 3, 8, 0, False),
    "t32": (128, 2, 2, 5, 32, 0, False),                  # the shipped token count
    "cross": (128, 2, 4, 3, 8, 24, False),                # a point condition: blocks 0 and 2 cross-attend to 24 condition tokens
    "narrow": (128, 8, 2, 3, 8, 0, False),                # head width 16
    "row7": (128, 2, 2, 3, 8, 0, True),                   # row 7 of a 9-row batch-shared table through step_ptr
}


def setup(tiny_cfg, name):
    hidden, heads, blocks, B, T, S, shared = CASES[name]
    model, x, t, _, _ = tt.make_case(tiny_cfg.score, hidden, heads, blocks, B, T, 1, None)
    model = model.cuda().eval()
    x = x.cuda().contiguous()
    g = torch.Generator().manual_seed(31)
    kv, extra = None, None
    if S:
        pts_cond = torch.randn(B, hidden, S, generator=g).cuda()
        extra, kv, S2 = model.condition_embedding(None, (pts_cond, 0.))
        assert S2 == S and sorted(kv) == [0, 2]
    if shared:
        ts = (torch.rand(9, generator=g) * 0.98 + 0.01).cuda()
        _, mod = model.time_table(ts)
        strides, step = (model.n_mod, 0), 7
    else:
        _, mod = model.time_table(t.cuda().float(), extra_c=extra)
        strides, step = (0, model.n_mod), None
    return model, x, mod, strides, step, kv, S


def runner(model, x, strides, step, kv, S):
    B, T, _ = x.shape

    def run(n, table):
        W = model._workspace(B, T)
        for k in it.STAGE_BUFFERS:
            W[k].fill_(float("nan"))
        p = model.plan(B, T, table, strides[0], strides[1], kv_cond=kv, cond_tokens=S)
        assert not p.fold, "the stage audit is for unfolded plans"
        if n is not None:
            p.blocks = n
        eps = model._run(p, x, step)
        torch.cuda.synchronize()
        return dict({k: W[k].clone() for k in it.STAGE_BUFFERS}, eps=eps)
    return run


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_stage_within_the_bound_of_its_kernel(tiny_cfg, name):
    model, x, mod, strides, step, kv, S = setup(tiny_cfg, name)
    hidden, heads, blocks, B, T, _, _ = CASES[name]
    dims = (B, T, hidden, heads, blocks, model.z_dim)
    worst, two = it.audit_score_stages(runner(model, x, strides, step, kv, S), it.score_panels(model, kv), dims, x, mod, strides[1], step)
    print("%-8s two-kernel route per block: %s" % (name, two))
    for k in sorted(worst):
        print("%-8s %-44s %.4f" % (name, k, worst[k]))
        WORST[k] = max(WORST.get(k, 0.0), worst[k])
    bad = {k: v for k, v in it.ratios(worst).items() if not v <= 1.0}
    assert not bad, bad
    # the plan as the product runs it computes what the stages were held to
    want = model.forward_table_row(x, step, mod) if step is not None else None
    if want is not None:
        assert torch.equal(want, runner(model, x, strides, step, kv, S)(None, mod)["eps"])


def test_a_residual_gemm_under_a_zero_gate_returns_its_residual():
    """Once per GEMM route the Score cases' residual GEMMs take (fc_o: K = D, mlp.out: K = 4 D): out = resid + 0 (x w^T + b) == resid."""
    from ldt_amd import ops
    from ldt_amd._lib import EPI_RESID_F32
    seen = {}
    for hidden, heads, blocks, B, T, _, _ in CASES.values():
        for K in (hidden, 4 * hidden):
            seen.setdefault(tuple(ops.gemm_route(EPI_RESID_F32, B * T, hidden, K)), (B, T, hidden, K))
    assert seen
    g = torch.Generator().manual_seed(3)
    for route, (B, T, D, K) in seen.items():
        M = B * T
        xb, w = torch.randn(M, K, generator=g).bfloat16().cuda(), (torch.randn(D, K, generator=g) / K ** 0.5).bfloat16().cuda()
        b, resid = torch.randn(D, generator=g).cuda(), torch.randn(M, D, generator=g).cuda()
        for gate, stride, rps in ((torch.zeros(B, D, device="cuda"), D, T), (torch.zeros(1, D, device="cuda"), 0, M)):
            out = resid.clone()
            ops.gemm_bf16(xb, w, b, EPI_RESID_F32, out=out, resid=out, gate=gate, gate_sample_stride=stride, rows_per_sample=rps)
            assert torch.equal(out, resid), "route %s, M %d N %d K %d: a zero gate does not return the residual" % (route, M, D, K)


def test_zz_margins():
    for k in sorted(WORST):
        print("%-52s %.4f" % (k, WORST[k]))
    assert all(v <= 1.0 for v in it.ratios(WORST).values())
