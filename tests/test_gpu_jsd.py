"""GPU (-m gpu): the JSD metric on the HIP path — ldt_occupancy_grid and the `ldt_amd.metrics` functions on top of it against
tests/golden/jsd.npz (the reference's counters on two seeded cloud sets, one inside radius 0.45 and one reaching radius 1 where the
boundary cells collect; captured by tools/golden/gen_hybrid_eval_golden.py, which asserts that no point's nearest cell hangs on a tie),
and against a float64 brute force on the device's own inputs.  The histograms are integers: every comparison of counts is exact and no
point is left out."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def jsd_golden():
    z = np.load(os.path.join(GOLDEN, "jsd.npz"))
    return {k: np.asarray(z[k]) for k in z.files}


def brute_force(pts, cells):
    """float64 (dx^2 + dy^2) + dz^2 over every (point, cell) pair in torch on the device, the lowest index among the minima:
    -> (counters, bernoulli) int64 [G]."""
    S, n, G = pts.shape[0], pts.shape[1], cells.shape[0]
    c = cells.double()
    counters = torch.zeros(G, dtype=torch.int64, device=pts.device)
    bern = torch.zeros(G, dtype=torch.int64, device=pts.device)
    order = torch.arange(G, device=pts.device)
    for s in range(S):
        d = pts[s].double()[:, None, :] - c[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        lowest = d2.min(dim=1, keepdim=True).values
        arg = torch.where(d2 == lowest, order[None, :], G).min(dim=1).values
        hist = torch.bincount(arg, minlength=G)
        counters += hist
        bern += (hist > 0).long()
    return counters, bern


@pytest.mark.parametrize("in_sphere", [True, False])
@pytest.mark.parametrize("name", ["in", "out"])
def test_occupancy_counts_equal_the_reference(name, in_sphere):
    from ldt_amd import metrics as M
    g = jsd_golden()
    tag = "sphere" if in_sphere else "cube"
    pcs, res = g["pcs_" + name], int(g["resolution"])
    counters, bern = M.occupancy_counts(pcs, res, in_sphere)
    want_c, want_b = g["%s/%s/grid_counters" % (name, tag)], g["%s/%s/bernoulli" % (name, tag)]
    assert counters.dtype == np.int64 and counters.shape == want_c.shape
    assert int(counters.sum()) == pcs.shape[0] * pcs.shape[1]                     # every point is counted once
    print("occupancy %s/%s: %d cells, %d occupied, counters differing %d, bernoulli differing %d" % (
        name, tag, len(want_c), int((counters > 0).sum()), int((counters != want_c.astype(np.int64)).sum()), int((bern != want_b).sum())))
    assert np.array_equal(counters, want_c.astype(np.int64))
    assert np.array_equal(bern, want_b)
    # through the reference's function: (acc_entropy, float64 counters); a device tensor and a numpy array alike
    acc, grid_counters = M.entropy_of_occupancy_grid(torch.from_numpy(pcs).cuda(), res, in_sphere)
    assert isinstance(acc, float) and grid_counters.dtype == np.float64 and np.array_equal(grid_counters, want_c)
    print("acc_entropy %.17g vs the reference's %.17g" % (acc, float(g["%s/%s/acc_entropy" % (name, tag)])))
    assert abs(acc - float(g["%s/%s/acc_entropy" % (name, tag)])) <= 1e-12
    acc2, grid_counters2 = M.entropy_of_occupancy_grid(pcs, res, in_sphere)
    assert acc2 == acc and np.array_equal(grid_counters2, grid_counters)          # a second run: the same bits


def test_jsd_between_point_cloud_sets_golden():
    from ldt_amd import metrics as M
    g = jsd_golden()
    res = int(g["resolution"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        jsd = M.jsd_between_point_cloud_sets(g["pcs_in"], g["pcs_out"], res)
    print("JSD %.17g vs the reference's %.17g" % (jsd, float(g["jsd"])))
    assert abs(jsd - float(g["jsd"])) <= 1e-12
    assert M.jsd_between_point_cloud_sets(torch.from_numpy(g["pcs_in"]).cuda(), torch.from_numpy(g["pcs_out"]).cuda(), res) == jsd
    assert abs(M.jsd_between_point_cloud_sets(g["pcs_out"], g["pcs_out"]) - float(g["jsd_self"])) <= 1e-12       # resolution defaults to 28
    # the two warnings of `verbose` (the 'out' set leaves the unit cube and the unit sphere); silent otherwise
    with pytest.warns(UserWarning) as rec:
        M.entropy_of_occupancy_grid(g["pcs_out"][:2], res, True, verbose=True)
    assert sorted(str(w.message) for w in rec) == ["Point-clouds are not in unit cube.", "Point-clouds are not in unit sphere."]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M.entropy_of_occupancy_grid(g["pcs_out"][:2], res, True)
        M.entropy_of_occupancy_grid(g["pcs_in"][:2], res, True, verbose=True)


def test_occupancy_grid_ragged_ties_and_accumulation():
    """S = 3 clouds of n = 1000 points (not a multiple of the workgroup's points per pass) on G = 777 random cells (not a multiple of the
    LDS tile) and on the 28^3 grid, against the float64 brute force; duplicated cells make exact ties, which the lowest index wins;
    given histograms are added to."""
    from ldt_amd import metrics as M, ops
    gen = torch.Generator().manual_seed(21)
    pts = (torch.randn(3, 1000, 3, generator=gen) * 0.3).cuda()
    cells = (torch.rand(777, 3, generator=gen) - 0.5)
    cells[700:] = cells[:77]                                                      # 77 exact ties
    cells = cells.cuda()
    counters, bern = ops.occupancy_grid(pts, cells)
    want_c, want_b = brute_force(pts, cells)
    assert counters.dtype == torch.int32 and counters.shape == (777,)
    assert torch.equal(counters.long(), want_c) and torch.equal(bern.long(), want_b)
    assert int(counters[700:].sum()) == 0 and int(counters.sum()) == 3000 and int(bern.max()) <= 3
    grid = torch.from_numpy(M.unit_cube_grid_point_cloud(28)[0].reshape(-1, 3)).cuda()
    c28, b28 = ops.occupancy_grid(pts, grid)
    w28, wb28 = brute_force(pts, grid)
    assert torch.equal(c28.long(), w28) and torch.equal(b28.long(), wb28)
    again_c, again_b = ops.occupancy_grid(pts, grid)
    assert torch.equal(again_c, c28) and torch.equal(again_b, b28)
    # n larger than one pass of the workgroup (256 threads x 8 points), one cloud at a time: the same histogram
    big = (torch.randn(1, 2500, 3, generator=gen) * 0.3).cuda()
    cb, bb = ops.occupancy_grid(big, cells)
    wcb, wbb = brute_force(big, cells)
    assert torch.equal(cb.long(), wcb) and torch.equal(bb.long(), wbb)
    # accumulation into given histograms
    acc_c, acc_b = counters.clone(), bern.clone()
    out_c, out_b = ops.occupancy_grid(big, cells, acc_c, acc_b)
    assert out_c is acc_c and torch.equal(acc_c, counters + cb) and torch.equal(acc_b, bern + bb)
    with pytest.raises(ValueError):
        ops.occupancy_grid(pts, cells, torch.zeros(5, dtype=torch.int32, device="cuda"), None)
    with pytest.raises(ValueError):
        ops.occupancy_grid(pts[..., :2], cells)
