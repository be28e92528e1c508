"""GPU (-m gpu): the prior-row gradient alone (ldt_rows_gather_sum: csrc/score_bwd.hip), the backward of InitialSet's learned prior rows:
dprior[r] = the sum over the samples that hold row r of their row's gradient, in the order of b.  Reference and bound:
tests/decoder_train_checks.py (held against torch.autograd on the reference's own selection by test_decoder_train_host.py).

  * per element against float64, with and without a keep mask, from a strided dy inside guard bands
  * exact: a row one sample holds is that sample's row bit for bit; a row no sample kept is exactly 0; an index outside [0, N) is skipped
  * a second call repeats bit for bit

Before ldt_rows_gather_sum existed every test here ended at the missing `ops.rows_gather_sum`."""
import pytest
import torch

import decoder_train_checks as dc
import kernel_checks as kc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,R,N,C,masked", [(3, 64, 64, 64, False), (2, 320, 300, 128, True), (5, 7, 3, 300, True), (1, 1, 1, 1, False)])
def test_rows_gather_sum_per_element(B, R, N, C, masked):
    from ldt_amd import ops
    g = torch.Generator().manual_seed(B + R + N + C)
    if masked:                                                           # every sample keeps N of the R rows, each its own
        keep = torch.zeros(B, R, dtype=torch.bool)
        for b in range(B):
            keep[b, torch.randperm(R, generator=g)[:N]] = True
        keep[:, R - 1] = False                                           # a row nobody kept (N < R)
        for b in range(B):
            spare = torch.nonzero(~keep[b, :R - 1]).flatten()
            keep[b, spare[:N - int(keep[b].sum())]] = True
        assert bool((keep.sum(1) == N).all())
    else:
        assert R == N
        keep = torch.ones(B, R, dtype=torch.bool)
    src = ops.prior_row_map(keep)
    big, wide = kc.guarded(B * N, C + 8, float("nan"), "cuda")
    dy = torch.randn(B * N, C, generator=g)
    wide[:, :C] = dy.cuda()
    out = ops.rows_gather_sum(wide[:, :C], src.cuda(), N)
    kc.assert_guard_intact(big, B * N * (C + 8), "rows_gather_sum")
    ref, tol = dc.rows_gather_sum_ref(dy, src, N)
    r = kc.assert_elementwise(out.cpu(), ref, tol, "rows_gather_sum")
    print("train-kernel rows_gather_sum B%d R%d N%d C%d masked=%d: max err/tol %.3f" % (B, R, N, C, masked, r))
    held = keep.sum(0)
    assert bool((out.cpu()[held == 0] == 0).all()) and (not masked or int((held == 0).sum()) >= 1)
    for r_ in torch.nonzero(held == 1).flatten().tolist():               # one holder: its row bit for bit
        b = int(torch.nonzero(keep[:, r_]).flatten()[0])
        assert torch.equal(out[r_].cpu(), dy[b * N + int(src[b, r_])])
    assert torch.equal(ops.rows_gather_sum(wide[:, :C], src.cuda(), N), out)


def test_an_index_outside_the_sample_is_skipped():
    from ldt_amd import ops
    dy = torch.arange(24, dtype=torch.float32).view(6, 4).cuda()         # B 2, N 3
    src = torch.tensor([[0, 3, -1, 2], [7, 1, -5, 2]], dtype=torch.int32).cuda()
    out = ops.rows_gather_sum(dy, src, 3).cpu()
    want = torch.stack([dy[0].cpu(), dy[4].cpu(), torch.zeros(4), dy[2].cpu() + dy[5].cpu()])
    assert torch.equal(out, want)
    with pytest.raises(ValueError, match=r"not \[B \* N, C\]"):
        ops.rows_gather_sum(dy, src, 4)
    torch.cuda.synchronize()
