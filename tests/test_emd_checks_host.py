"""CPU: what test_gpu_emd_exact.py and test_gpu_metrics.py rest on (emd_checks.py), checked with the reference alone.

  * emd_ref64 is the oracle's algorithm: equal to O.emd_approxmatch_cost (fp32) within 1e-6 on the random case table;
  * the closed forms of the probes: the lattice probes' sum of displacements within 1e-8 of emd_ref64, the single-point probes' delta within 1e-6;
  * every planted fault (a point that contributes no cost, each of the nine levels skipped, the multipliers exchanged, the pair indices
    transposed, remainL stale from k = 1024) moves some case by more than 3 EMD_REL: the conditions on the inputs that make the GPU tests
    able to fail, and the cap on EMD_REL;
  * the many-pairs clouds are well conditioned in fp32;
  * on the golden clouds the nearest-reference and nearest-neighbour gaps exceed 100 EMD_REL, so the counts the GPU test compares are
    unambiguous."""
import math

import pytest
import torch

import emd_checks as ec
from conftest import load_golden

SMALL = [c for c in ec.TABLE + ec.SWEEP if c[0] * c[1] <= 1 << 17]
BIG_ONE = (1500, 700, 0.5)                  # n > 1024 on one side, n != m: a single pair of it costs 0.1 s


def rel(a, b):
    return ((a.double() - b.double()).abs() / b.double().abs()).reshape(-1)


def moved(fault, base):
    """Largest relative effect of a planted fault over the pairs of a case."""
    return float(rel(fault, base).max())


@pytest.fixture(scope="module")
def big_one():
    x, y, ref = ec.case_reference(BIG_ONE)              # its first pair
    return x[:1], y[:1], ref[0, :1]


def test_emd_rel_is_a_power_of_two_under_the_cap():
    assert math.log2(ec.EMD_REL) == round(math.log2(ec.EMD_REL))
    assert ec.EMD_REL <= 2.0 ** -15                     # a third of 9e-5, the effect of one forgotten point at 2048 random points


@pytest.mark.parametrize("case", ec.TABLE + ec.SWEEP, ids=ec.case_id)
def test_ref64_equals_the_fp32_oracle(case):
    from oracle import ldt_oracle as O
    x, y, ref = ec.case_reference(case)
    pairs = 1 if case[0] * case[1] >= 1 << 20 else 2    # the oracle loops over pairs in fp32
    want = ref[:pairs] if ref.dim() == 1 else ref.diagonal()[:pairs]
    got = O.emd_approxmatch_cost(x[:pairs], y[:pairs])
    r = float(rel(got, want).max())
    print("emd_ref64 vs fp32 oracle %-20s %.2e" % (ec.case_id(case), r))
    assert r <= 1e-6


@pytest.mark.parametrize("n", ec.LATTICE_SIZES)
def test_lattice_probe_closed_form(n):
    x, y, total, disp = ec.lattice_probe(n)
    assert abs(float(ec.emd_ref64(x, y)[0]) - total) <= 1e-8 * total
    assert float(disp.max()) < 0.05                                                   # far below the spacing
    assert float((disp[1024:] - disp[:n - 1024]).abs().min()) > 1e-3 if n > 1024 else True      # distinct among one lane's points
    assert float(disp.min()) / total >= 3 * ec.EMD_REL, "n = %d: raise the smallest displacement" % n
    # a lane that forgets any one of its points is caught at every owner index
    for k in (i % n for i in ec.OWNER_INDICES):
        assert float(disp[k]) / total > 3 * ec.EMD_REL


def test_single_point_probe_closed_form():
    n = 1100
    x, y, want, owners = ec.single_point_probes(n)
    assert sorted(set(k for k, _ in owners)) == sorted(set(i % n for i in ec.OWNER_INDICES)) and len(owners) == 36
    sel = [6 * i + (i + 1) % 6 for i in range(6)]       # every k and every l once
    got = ec.emd_ref64(x[sel], y[sel])
    assert float(rel(got, want[sel]).max()) <= 1e-6
    for i in sel:                                       # the displaced point is x_k's copy at position l, everything else coincides
        k, l = owners[i]
        d = (y[i, l].double() - x[i, k].double()).norm()
        assert abs(float(d) - float(want[i])) < 1e-12 and float(want[i]) > 0.009
        others = torch.ones(n, dtype=torch.bool); others[l] = False
        assert torch.equal(y[i, others].sort(0).values, x[i, torch.arange(n) != k].sort(0).values)


@pytest.mark.parametrize("k", [0, 1024, -1])
def test_planted_dropped_point(big_one, k):
    x, y, base = big_one
    assert moved(ec.emd_ref64(x, y, drop_point=k % x.shape[1]), base) > 3 * ec.EMD_REL


@pytest.mark.parametrize("j", ec.LEVELS)
def test_planted_skipped_level(j):
    """For each level the table holds a case on which that level matters."""
    worst = {}
    for case in SMALL:
        x, y, base = ec.case_reference(case)
        worst[ec.case_id(case)] = moved(ec.emd_ref64(x, y, True, skip_level=j), base)
    best = max(worst, key=worst.get)
    print("level j = %2d matters most on %-14s: %.2e" % (j, best, worst[best]))
    assert worst[best] > 3 * ec.EMD_REL


def test_planted_skipped_level_where_a_lane_owns_two_points():
    """The first and the last level also matter on a case with n > 1024 (with equal masses: at 1500 x 700 everything is matched before j = -1)."""
    x, y, ref = ec.case_reference((1025, 1025, 0.5))
    for j in (7, -1):
        assert moved(ec.emd_ref64(x[:1], y[:1], skip_level=j), ref[0, :1]) > 3 * ec.EMD_REL, j


@pytest.mark.parametrize("case", [(100, 230, 1.0), (300, 100, 1.0), BIG_ONE], ids=ec.case_id)
def test_planted_swapped_multipliers(case):
    x, y, base = ec.case_reference(case)
    assert moved(ec.emd_ref64(x[:1], y[:1], swap_multipliers=True), base[0, 0]) > 3 * ec.EMD_REL


def test_planted_transposed_pairs():
    for case in ((17, 17, 1.0), (100, 230, 1.0)):
        x, y, base = ec.case_reference(case)
        assert base.shape == (2, 3)                     # S != R
        t = ec.emd_ref64(x, y, True, transpose_pairs=True)
        assert int((rel(t, base) > 3 * ec.EMD_REL).sum()) == 4      # every pair but the first and the last sits elsewhere
    x, y = ec.many_pairs_case()
    base = ec.emd_ref64(x, y, True)
    assert moved(ec.emd_ref64(x, y, True, transpose_pairs=True), base) > 3 * ec.EMD_REL
    v = base.reshape(-1)                                # pairs 4096 .. 4224 written where pairs 0 .. 128 belong, or not at all
    assert float(rel(v[4096:], v[:129]).min()) > 3 * ec.EMD_REL


def test_planted_stale_remain(big_one):
    x, y, base = big_one
    assert moved(ec.emd_ref64(x, y, stale_remain=True), base) > 3 * ec.EMD_REL
    xs, ys, small = ec.case_reference((300, 100, 1.0))  # no point from 1024 on: the fault is not there to see
    assert torch.equal(ec.emd_ref64(xs, ys, True, stale_remain=True), small)


def test_many_pairs_clouds_are_well_conditioned():
    x, y = ec.many_pairs_case()
    assert x.shape == (65, 8, 3) and y.shape == (65, 8, 3)
    base = ec.emd_ref64(x, y, True)
    r = moved(ec.emd_ref64(x, y, True, dtype=torch.float32), base)
    print("many pairs: fp32 evaluation vs float64 %.2e" % r)
    assert r <= ec.EMD_REL / 4


def test_degenerate_cases_have_small_costs():
    for name, x, y, diameter in ec.degenerate_cases():
        cost = float(ec.emd_ref64(x, y)[0])
        assert diameter > 1.0 and cost >= 0.0, name
        if name.startswith("permuted"):
            assert cost < 1e-4 * x.shape[1] * diameter, name


def test_golden_gaps_decide_the_counts():
    a, _ = load_golden("metrics_cd")
    ref, smp = a["ref"], a["smp"]
    assert ref.shape[1:] == (96, 3) and smp.shape[1:] == (96, 3) and {ref.shape[0], smp.shape[0]} == {12, 13}
    M_rs, M_rr, M_ss = ec.golden_matrices(ref, smp)
    cov_gap = ec.nearest_gaps(M_rs.t())                 # the two nearest references of any sample: decides cov
    nn_gap = ec.nearest_gaps(ec.stacked_1nn(M_rr, M_rs, M_ss).t())     # knn takes the nearest per column; the approximate EMD is not symmetric
    print("golden clouds: smallest relative gap, nearest reference %.2e, nearest neighbour %.2e" % (cov_gap, nn_gap))
    assert cov_gap > 100 * ec.EMD_REL and nn_gap > 100 * ec.EMD_REL
