"""GPU (-m gpu): the backward of the posterior draw and the KL term alone, per element (ldt_reparam_kl_bwd: csrc/eval_loss.hip).  Cases,
the float64 reference (equal to autograd over the reference's expressions: test_topdown_train_host.py) and the bound of a few fp32
roundings per term: tests/topdown_train_checks.py.

  * (rows, z) = (24, 40) in the 16-byte form, (7, 5) in the scalar form, (512, 20) the shipped rows x z; d_eps dense and as a column
    slice of a wider buffer (at a 16-byte aligned and at an unaligned column: both forms of the kernel give the same bits)
  * logvar below lo, above hi and exactly on both bounds: exact zeros outside the clamp, the gradient on the bounds themselves
  * eps is recomputed with the bits of ldt_reparam (read back through dmu at kl_scale 1, d_eps 0)
  * kl_scale 0 leaves the draw's gradient alone, d_eps 0 the KL term's alone
  * a second call repeats bit for bit; the refusals

Before ldt_reparam_kl_bwd existed every test here ended at the missing `ops.reparam_kl_bwd`."""
import pytest
import torch

import kernel_checks as kc
import topdown_train_checks as tc

pytestmark = pytest.mark.gpu
LO, HI = -6.0, 10.0


@pytest.mark.parametrize("rows,z", tc.RKB_SHAPES)
@pytest.mark.parametrize("kl_scale", [0.05, 0.0])
def test_reparam_kl_bwd_per_element(rows, z, kl_scale):
    from ldt_amd import ops
    post, noise, d_eps = tc.rkb_case(rows, z, LO, HI)
    ref, tol = tc.reparam_kl_bwd_closed(post, noise, d_eps, kl_scale, LO, HI)
    got = ops.reparam_kl_bwd(post.cuda(), noise.cuda(), d_eps.cuda(), kl_scale, LO, HI)
    assert tuple(got.shape) == (rows, 2 * z) and got.dtype == torch.float32
    r = kc.assert_elementwise(got.cpu(), ref, tol, "reparam_kl_bwd rows %d z %d kl_scale %g" % (rows, z, kl_scale))
    print("train-kernel reparam_kl_bwd rows %d z %d kl_scale %g  max err/tol %.3f" % (rows, z, kl_scale, r))
    raw = post[:, z:]
    out = (raw < LO) | (raw > HI)
    assert bool(out.any()) and bool((got.cpu()[:, z:][out] == 0).all())              # exact zeros outside the clamp
    on = (raw == LO) | (raw == HI)
    assert bool(on.any()) and (kl_scale == 0 or bool((got.cpu()[:, z:][on] != 0).all()))
    assert torch.equal(ops.reparam_kl_bwd(post.cuda(), noise.cuda(), d_eps.cuda(), kl_scale, LO, HI), got)
    # d_eps as a column slice of the [rows, L z] buffer the step keeps: an aligned column (the same form of the kernel when z % 4 == 0) and
    # an unaligned one (the scalar form): the same bits
    for col in (4 * z, 3):
        wide = torch.full((rows, 6 * z + 3), float("nan"), device="cuda")
        wide[:, col:col + z] = d_eps.cuda()
        assert torch.equal(ops.reparam_kl_bwd(post.cuda(), noise.cuda(), wide[:, col:col + z], kl_scale, LO, HI), got), col


@pytest.mark.parametrize("rows,z", tc.RKB_SHAPES)
def test_eps_is_recomputed_with_the_bits_of_reparam(rows, z):
    """kl_scale 1, d_eps 0: dmu = fma(1, eps, 0) = eps."""
    from ldt_amd import ops
    post, noise, _ = tc.rkb_case(rows, z, LO, HI)
    post_d, noise_d = post.cuda(), noise.cuda()
    eps = torch.empty((rows, z), device="cuda")
    ops.reparam(post_d, noise_d, eps, LO, HI)
    eps2 = torch.empty_like(eps)
    ops.reparam_kl(post_d, noise_d, eps2, LO, HI, rows)
    got = ops.reparam_kl_bwd(post_d, noise_d, torch.zeros_like(eps), 1.0, LO, HI)
    assert torch.equal(eps2, eps) and torch.equal(got[:, :z], eps)


def test_the_two_paths_alone_and_the_refusals():
    from ldt_amd import ops
    from ldt_amd._lib import LdtHipError
    rows, z = 24, 40
    post, noise, d_eps = tc.rkb_case(rows, z, LO, HI)
    post_d, noise_d, de = post.cuda(), noise.cuda(), d_eps.cuda()
    rec = ops.reparam_kl_bwd(post_d, noise_d, de, 0.0, LO, HI)
    assert torch.equal(rec[:, :z], de)                                               # dmu = d_eps: the draw passes it through
    kl = ops.reparam_kl_bwd(post_d, noise_d, torch.zeros_like(de), 0.05, LO, HI)
    ref, tol = tc.reparam_kl_bwd_closed(post, noise, torch.zeros_like(d_eps), 0.05, LO, HI)
    kc.assert_elementwise(kl.cpu(), ref, tol, "the KL term alone")
    live = ((post[:, z:] >= LO) & (post[:, z:] <= HI)).cuda()
    assert bool((kl[:, z:][live] != rec[:, z:][live]).all())                         # -kl_scale / 2 is there whatever eps is
    with pytest.raises(ValueError, match="d_eps \\[rows, z\\] with unit column stride"):
        ops.reparam_kl_bwd(post_d, noise_d, de[:, :8], 0.05, LO, HI)
    with pytest.raises(ValueError, match="not \\[rows, 2z\\]"):
        ops.reparam_kl_bwd(post_d[:, :79].contiguous(), noise_d, de, 0.05, LO, HI)
    with pytest.raises(TypeError):
        ops.reparam_kl_bwd(post_d.double(), noise_d, de, 0.05, LO, HI)
    with pytest.raises(LdtHipError, match="no CPU fallback"):
        ops.reparam_kl_bwd(post_d, noise, de, 0.05, LO, HI)
    torch.cuda.synchronize()
