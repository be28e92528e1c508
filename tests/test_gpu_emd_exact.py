"""GPU (-m gpu): the approximate-matching EMD kernel (csrc/metrics.hip emd_approx_kernel, behind ldt_emd_approx) per pair and per point.

Every pair's cost is held to emd_checks.EMD_REL against the float64 restatement emd_ref64 (never against the kernel), on
  * the random case table: one lane per point and several (n > 1024), n != m with integer mass ratios, single points, batched and pairwise
    (row-major [S][R]) launches, and the scales at which each of the nine annealing levels carries mass;
  * lattice probes whose cost is the sum of the displacements, up to n + m = 7680 (all of the 150 KB of LDS): no CPU annealing;
  * single-point probes that attribute the cost to one owner lane on each side;
  * 4225 pairs, of which 4096 .. 4224 are second iterations of the grid-stride loop on used LDS;
  * identical / repeated clouds, where the cost is near 0;
and the call is held to its contract: same bits twice, nothing written past npairs, inputs unchanged, LDT_ESHAPE past the LDS limit.
test_emd_checks_host.py proves on the CPU that every planted fault moves some case by more than 3 EMD_REL."""
import collections
import time

import pytest
import torch

import emd_checks as ec

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)          # worst err / bound per case class (test_zz_margins)
T0 = [None]


@pytest.fixture(scope="module", autouse=True)
def _mods():
    T0[0] = time.time()
    assert torch.cuda.is_available()


def hold(got, want, what, cls, floor=0.0):
    """|got - want| <= EMD_REL * want (+ floor) for every pair; prints the worst ratio first.  -> worst err / bound."""
    got, want = got.detach().cpu().double().reshape(-1), want.double().reshape(-1)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), (what, got.shape, want.shape)
    err = (got - want).abs()
    bound = ec.EMD_REL * want.abs() + floor
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    i = int(ratio.argmax())
    print("emd %-34s pairs %4d  worst |err|/ref %.3e  err/bound %.3f (pair %d)"
          % (what, got.numel(), float((err / want.abs().clamp_min(1e-300)).max()), float(ratio[i]), i))
    RATIOS[cls] = max(RATIOS[cls], float(ratio[i]))
    assert bool((err <= bound).all()), "%s: pair %d got %r, want %r, |err|/ref %.3e > EMD_REL %.3e" % (
        what, i, float(got[i]), float(want[i]), float(err[i] / want[i].abs()), ec.EMD_REL)
    return float(ratio[i])


@pytest.mark.parametrize("case", ec.TABLE + ec.SWEEP, ids=ec.case_id)
def test_random_case_table(case):
    from ldt_amd import ops
    x, y, ref = ec.case_reference(case)
    cls = "sweep" if case in ec.SWEEP else ("n > 1024" if max(case[0], case[1]) > 1024 else "n <= 1024")
    xd, yd = x.cuda(), y.cuda()
    if ref.dim() == 1:                                                      # the two large cases: batched only
        hold(ops.emd_approx(xd, yd), ref, ec.case_id(case) + " batched", cls)
        return
    hold(ops.emd_approx(xd[:2], yd[:2].contiguous()), ref.diagonal(), ec.case_id(case) + " batched", cls)
    pw = ops.emd_approx(xd, yd, pairwise=True)
    assert pw.shape == ref.shape                                           # row-major [S][R]
    hold(pw, ref, ec.case_id(case) + " pairwise", cls)


@pytest.mark.parametrize("n", ec.LATTICE_SIZES)
def test_lattice_probe(n):
    from ldt_amd import ops
    x, y, total, disp = ec.lattice_probe(n)
    assert float(disp.min()) / total >= 3 * ec.EMD_REL                      # a lane that forgets one point is outside the bound
    hold(ops.emd_approx(x.cuda(), y.cuda()), torch.tensor([total], dtype=torch.float64), "lattice %d" % n, "lattice")


def test_single_point_probes():
    from ldt_amd import ops
    x, y, want, owners = ec.single_point_probes(2048)
    got = ops.emd_approx(x.cuda(), y.cuda())
    for (k, l), g, w in zip(owners, got.cpu().tolist(), want.tolist()):
        assert abs(g - w) <= ec.EMD_REL * w, "owner lanes k = %d, l = %d: got %r, want %r" % (k, l, g, w)
    hold(got, want, "single point, 36 owners", "single point")


def test_more_than_4096_pairs():
    from ldt_amd import ops
    x, y = ec.many_pairs_case()
    ref = ec.emd_ref64(x, y, pairwise=True)
    got = ops.emd_approx(x.cuda(), y.cuda(), pairwise=True)
    assert got.numel() == 4225
    hold(got.reshape(-1)[:4096], ref.reshape(-1)[:4096], "4225 pairs, first pass", "many pairs")
    hold(got.reshape(-1)[4096:], ref.reshape(-1)[4096:], "4225 pairs, second pass", "many pairs")


def test_contract():
    from ldt_amd import _lib, ops
    lib = _lib.lib()
    x, y, ref = ec.case_reference((100, 230, 1.0))
    xd, yd = x.cuda(), y.cuda()
    x0, y0 = xd.clone(), yd.clone()
    S, R, n, m = x.shape[0], y.shape[0], x.shape[1], y.shape[1]
    sentinel = -12345.5
    outs = []
    for _ in range(2):
        out = torch.full((S * R + 64,), sentinel, device="cuda")
        _lib.check(lib.ldt_emd_approx(xd.data_ptr(), yd.data_ptr(), S, R, n, m, 1, out.data_ptr(), ops.stream_ptr()), "ldt_emd_approx")
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])                                    # two launches: the same bits
    assert bool((outs[0][S * R:] == sentinel).all())                        # nothing past npairs
    assert torch.equal(xd, x0) and torch.equal(yd, y0)                      # the inputs are unchanged
    hold(outs[0][:S * R], ref, "contract 100x230", "n <= 1024")
    small = lambda: hold(ops.emd_approx(xd[:2], yd[:2].contiguous()), ref.diagonal(), "valid call after an error", "n <= 1024")
    big = torch.zeros(1, 3841, 3, device="cuda")
    with pytest.raises(_lib.LdtHipError, match=r"status -2"):              # n + m = 7681: LDT_ESHAPE
        ops.emd_approx(big, big[:, :3840].contiguous())
    small()
    with pytest.raises(_lib.LdtHipError, match=r"status -2"):              # batched S != R
        ops.emd_approx(xd, yd)
    small()


def test_identical_and_coincident_clouds():
    from ldt_amd import ops
    for name, x, y, diameter in ec.degenerate_cases():
        ref = ec.emd_ref64(x, y)
        hold(ops.emd_approx(x.cuda(), y.cuda()), ref, name, "near-zero cost", floor=ec.EMD_REL * x.shape[1] * diameter)


def test_zz_margins():
    """Printed last (DESIGN.md section 3 quotes them): the worst err / bound per case class at emd_checks.EMD_REL."""
    print("EMD_REL = %.3e (2^%d)" % (ec.EMD_REL, round(torch.log2(torch.tensor(ec.EMD_REL)).item())))
    for k in sorted(RATIOS):
        print("worst err / bound, %-20s %.3f  (|err|/ref %.3e)" % (k + ":", RATIOS[k], RATIOS[k] * ec.EMD_REL))
    if T0[0] is not None:
        print("module run time %.1f s" % (time.time() - T0[0]))
    assert all(v <= 1.0 for v in RATIOS.values())
