"""The approximate-matching EMD (csrc/metrics.hip emd_approx_kernel, behind ldt_emd_approx) held per pair and per point: a float64
restatement of the annealing, probes whose cost is known in closed form, and the one relative bound a pair's cost is held to (used by
test_emd_checks_host.py, test_gpu_emd_exact.py and test_gpu_metrics.py).  Nothing here needs a GPU to import.

The reference is the project's own restatement of approxmatchkernel + matchcostkernel; parity with the CUDA original stays unpinned
(DESIGN.md section 3)."""
import math

import numpy as np
import torch

LEVELS = tuple(range(7, -2, -1))                       # level = -4^j, j = 7 .. -1
EPS9 = float(np.float32(1e-9))                         # the kernel's 1e-9f
OWNER_INDICES = (0, 63, 64, 1023, 1024, -1)            # wave edge, workgroup edge (a lane's second point), last point
LATTICE_SIZES = (1024, 1500, 2048, 3840)               # 3840 + 3840 points fill the 150 KB of LDS exactly

# One relative bound on a pair's cost, |kernel - emd_ref64| <= EMD_REL * emd_ref64: the next power of two at or above 4 x the worst
# ratio measured on the MI355X over the whole case table of test_gpu_emd_exact.py (the factor 4: other seeds, and the data-dependent
# rounding pattern of v_exp_f32).  It must stay at or below a third of the smallest planted-fault effect test_emd_checks_host.py proves.
# Measured worst |kernel - emd_ref64| / emd_ref64 per case class (test_gpu_emd_exact.py::test_zz_margins prints them):
#   table, n, m <= 1024    5.2e-7 (1024 x 1024 at scale 0.3; 2.3e-7 and below up to 300 points)
#   table, n or m > 1024   2.1e-6 (2048 x 2048 at scale 0.3; 1.1e-6 uniform, 9.1e-7 at 2050 x 1025, 5.6e-7 at 1025 x 1025)
#   level sweep            3.4e-7
#   lattice probes         1.0e-7 (3840 points; 8e-11 at 1024)
#   single-point probes    9.4e-8
#   4225 pairs             1.5e-7 (1.1e-7 on pairs 4096 .. 4224, the second pass)
#   near-zero cost         2.5e-7 of the reference where it is not 0 (below the absolute floor everywhere)
# 4 x 2.1e-6 = 8.6e-6 -> 2^-16 = 1.53e-5.  The smallest planted-fault effect proved on the host is 9.2e-5 (the smallest displacement of the
# 3840-point lattice probe over the sum), so the cap is 3.1e-5.
EMD_REL = 2.0 ** -16


def _pair_indices(S, R, pairwise, transpose_pairs):
    if not pairwise:
        assert S == R, "batched mode pairs cloud b with cloud b"
        i = torch.arange(S)
        return i, i
    p = torch.arange(S * R)
    if transpose_pairs:                                # the planted fault: the fast index taken for the slow one, kept in bounds
        return p % S, p // S                           # (p % R, p / R for p / R, p % R; the output read as [R][S])
    return p // R, p % R


def emd_ref64(x, y, pairwise=False, *, drop_point=None, skip_level=None, swap_multipliers=False, transpose_pairs=False,
              stale_remain=False, dtype=torch.float64, budget=1 << 24):
    """The annealing of approxmatchkernel followed by matchcostkernel in float64 on the given coordinates: x [S, n, 3], y [R, m, 3] ->
    float64 [S] (pairs (x[b], y[b])) or [S, R] (pairwise, row-major).  Vectorised over pairs, `budget` elements of the n x m plane at a time.
    Per pair: masses multiL, multiR by integer division, nine levels -4^j (j = 7 .. -1), the 1e-9 terms and the clamps of the kernel, and
    cost = sum over levels of sum_{k,l} w(k,l) sqrt(d2(k,l)).
    The keyword arguments plant faults for the host tests: drop_point = k (point k of x contributes no cost), skip_level = j,
    swap_multipliers, transpose_pairs (see _pair_indices), stale_remain (remainL is not updated for k >= 1024)."""
    x, y = torch.as_tensor(x).to(dtype), torch.as_tensor(y).to(dtype)
    S, n, _ = x.shape
    R, m, _ = y.shape
    xi, yi = _pair_indices(S, R, pairwise, transpose_pairs)
    multiL, multiR = (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)
    if swap_multipliers:
        multiL, multiR = multiR, multiL
    out = torch.empty(xi.numel(), dtype=torch.float64)
    step = max(1, budget // (n * m))
    for p0 in range(0, xi.numel(), step):
        a, b = x[xi[p0:p0 + step]], y[yi[p0:p0 + step]]                     # [P, n, 3], [P, m, 3]
        d2 = torch.zeros(a.shape[0], n, m, dtype=dtype)
        for c in range(3):
            d2 += (b[:, None, :, c] - a[:, :, None, c]) ** 2
        dist = d2.sqrt()
        remainL = torch.full((a.shape[0], n), multiL, dtype=dtype)
        remainR = torch.full((a.shape[0], m), multiR, dtype=dtype)
        cost = torch.zeros(a.shape[0], n, dtype=dtype)
        for j in LEVELS:
            if j == skip_level:
                continue
            e = torch.exp(d2 * -(4.0 ** j))
            ratioL = remainL / (EPS9 + (e * remainR[:, None, :]).sum(2))
            sumr = (e * ratioL[:, :, None]).sum(1) * remainR
            ratioR = torch.clamp(remainR / (sumr + EPS9), max=1.0) * remainR
            remainR = torch.clamp(remainR - sumr, min=0.0)
            e *= ratioL[:, :, None]
            e *= ratioR[:, None, :]                                         # w(k, l)
            newL = torch.clamp(remainL - e.sum(2), min=0.0)
            if stale_remain:
                newL[:, 1024:] = remainL[:, 1024:]
            remainL = newL
            e *= dist
            cost += e.sum(2)
        if drop_point is not None:
            cost[:, drop_point] = 0.0
        out[p0:p0 + step] = cost.double().sum(1)
    return out.reshape(S, R) if pairwise else out


# ---- the random case table ----------------------------------------------------------------------------------------------------------
# (n, m, scale); scale None: uniform in the unit cube.  Gaussian clouds otherwise, the second cloud scaled 0.9 and offset.  100 x 230 runs
# with multiL = 2, 300 x 100 with multiR = 3.  SWEEP adds the scales at which each annealing level carries mass (test_emd_checks_host.py
# proves that every level matters on some case): dense small clouds for j = 7 .. 5, sparse ones for the low levels.
TABLE = ((1, 1, 1.0), (1, 5, 1.0), (5, 1, 1.0), (17, 17, 1.0), (64, 64, 0.5), (100, 230, 1.0), (300, 100, 1.0), (1024, 1024, 0.3),
         (1025, 1025, 0.5), (1500, 700, 0.5), (2050, 1025, 0.4), (2048, 2048, 0.3), (2048, 2048, None))
SWEEP = ((256, 256, 0.02), (256, 256, 0.05), (256, 256, 0.1), (256, 256, 0.25), (96, 96, 2.0), (64, 48, 4.0))
LARGE = 1 << 22          # n * m from which a float64 reference pair costs more than a second: three such pairs in all


def case_id(case):
    n, m, scale = case
    return "%dx%d-%s" % (n, m, "uniform" if scale is None else "%g" % scale)


def random_case(case, S=2, R=3):
    """-> x fp32 [S, n, 3], y fp32 [R, m, 3], seeded by the case itself."""
    n, m, scale = case
    g = torch.Generator().manual_seed(1000003 * n + 1009 * m + int(1000 * (scale or 0)))
    if scale is None:
        return torch.rand(S, n, 3, generator=g), torch.rand(R, m, 3, generator=g)
    x = torch.randn(S, n, 3, generator=g) * scale
    y = torch.randn(R, m, 3, generator=g) * (0.9 * scale) + torch.tensor([0.1, -0.05, 0.02]) * scale
    return x, y


def case_clouds(case):
    """The clouds a case runs on: pairwise [2] x [3], the batched call takes x[:2], y[:2] (the diagonal of the same reference matrix).  The
    two 2048 x 2048 cases hold three reference pairs between them: two batched pairs at scale 0.3, one pair on the uniform clouds."""
    n, m, scale = case
    if n * m >= LARGE:
        return random_case(case, 2, 2) if scale is not None else random_case(case, 1, 1)
    return random_case(case, 2, 3)


_REF = {}


def case_reference(case):
    """-> (x, y, float64 [S, R] reference matrix or, for the two large cases, the float64 [S] batched costs).  Computed once per process."""
    if case not in _REF:
        x, y = case_clouds(case)
        _REF[case] = (x, y, emd_ref64(x, y, pairwise=case[0] * case[1] < LARGE))
    return _REF[case]


# ---- probes with a cost known in closed form ----------------------------------------------------------------------------------------
def lattice_points(n):
    """Point k of the integer lattice 16 x 16 x ceil(n / 256), spacing 1: float64 [n, 3]."""
    k = torch.arange(n)
    return torch.stack([k % 16, (k // 16) % 16, k // 256], 1).double()


def lattice_delta(n, base=0.004):
    """The displacement of point k: distinct within a residue class of the 1024 lanes and far below the spacing."""
    k = torch.arange(n)
    return base * (1.0 + (k % 7).double() / 7.0 + (k // 1024).double())


def _unit_directions(n, g):
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return u / u.norm(dim=1, keepdim=True)


def lattice_probe(n, seed=0):
    """x on the lattice, y = perm(x + u_k delta_k).  At level j = 7 every point matches its own displaced copy completely (exp(-16384 d2) is 0
    for every other pair), so the cost is sum_k |y_k - x_k|.  -> (x fp32 [1, n, 3], y fp32 [1, n, 3], that sum in float64 on the fp32
    coordinates, the per-point displacements float64 [n])."""
    g = torch.Generator().manual_seed(7919 * n + seed)
    x = lattice_points(n)
    moved = (x + _unit_directions(n, g) * lattice_delta(n)[:, None]).float()
    disp = (moved.double() - x).norm(dim=1)
    perm = torch.randperm(n, generator=g)
    return x.float()[None], moved[perm][None].contiguous(), float(disp.sum()), disp


def single_point_probes(n, delta=0.01, seed=0):
    """One pair per (k, l) in OWNER_INDICES x OWNER_INDICES: x on the lattice, y = perm(x) with perm placing x_k at position l, and that one
    point displaced by delta.  Coincident points cost exactly 0 (d2 = 0), so the pair costs |y_l - x_k| up to the 1e-9 terms: the cost is
    attributed to one owner lane on each side.  -> (x fp32 [P, n, 3], y fp32 [P, n, 3], float64 [P] displacements, [(k, l), ...])."""
    g = torch.Generator().manual_seed(104729 * n + seed)
    idx = [i % n for i in OWNER_INDICES]
    base = lattice_points(n)
    xs, ys, want, owners = [], [], [], []
    for k in idx:
        for l in idx:
            perm = torch.randperm(n, generator=g)                         # y[i] = x[perm[i]]
            at = int(torch.nonzero(perm == k)[0])
            perm[at], perm[l] = perm[l].clone(), perm[at].clone()         # now perm[l] == k
            y = base[perm].clone()
            y[l] = (y[l] + _unit_directions(1, g)[0] * delta).float().double()
            xs.append(base.float()); ys.append(y.float())
            want.append(float((y[l] - base[k]).norm())); owners.append((k, l))
    return torch.stack(xs), torch.stack(ys), torch.tensor(want, dtype=torch.float64), owners


def many_pairs_case(S=65, R=65, n=8, seed=11):
    """More than 4096 pairs: the grid-stride loop runs pairs 4096 .. S R - 1 on LDS that pairs 0 .. S R - 4097 have used.  Every cloud is the
    2 x 2 x 2 lattice with its own Gaussian jitter of 0.1 (y in its own order), so every pair has its own cost and all of them are well
    conditioned.  Sparse random 8-point clouds are not: on about 2 % of such pairs one point pair matches almost completely at a high level,
    the fp32 remainder 1 - 0.99997 carries a relative error of 2e-3, and the next level normalises whole masses by it; there the fp32 oracle
    and the kernel both sit up to 1e-4 from float64, on the same pairs.  test_emd_checks_host.py holds the fp32 evaluation of these clouds
    to EMD_REL / 4."""
    g = torch.Generator().manual_seed(seed)
    base = torch.stack([torch.arange(n) % 2, (torch.arange(n) // 2) % 2, torch.arange(n) // 4], 1).double()
    x = base[None] + 0.1 * torch.randn(S, n, 3, generator=g, dtype=torch.float64)
    y = base[None] + 0.1 * torch.randn(R, n, 3, generator=g, dtype=torch.float64)
    y = torch.stack([y[r, torch.randperm(n, generator=g)] for r in range(R)])
    return x.float(), y.float()


def degenerate_cases(seed=3):
    """Costs near 0: x == y in another order, and clouds with repeated points.  -> [(name, x [1, n, 3], y [1, m, 3], diameter), ...]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in (96, 1300):
        x = torch.randn(1, n, 3, generator=g) * 0.5
        out.append(("permuted-%d" % n, x, x[:, torch.randperm(n, generator=g)].contiguous()))
    x = (torch.randn(1, 40, 3, generator=g) * 0.5).repeat(1, 5, 1)[:, torch.randperm(200, generator=g)].contiguous()
    y = torch.cat([x[:, :100], x[:, :100] + 0.05], 1)[:, torch.randperm(200, generator=g)].contiguous()
    out.append(("repeated-200", x, y))
    both = lambda a, b: torch.cat([a[0], b[0]]).double()
    return [(nm, a, b, float(torch.cdist(both(a, b), both(a, b)).max())) for nm, a, b in out]


def nearest_gaps(M):
    """Smallest relative gap between the two smallest entries of any row of M (float64): how far the matrix may move before an argmin does."""
    two = torch.topk(M, 2, dim=1, largest=False).values
    return float(((two[:, 1] - two[:, 0]) / two[:, 1]).min())


def golden_matrices(ref, smp):
    """The float64 EMD matrices of the golden clouds, each divided by n: M_rs [ref, smp], M_rr, M_ss."""
    n = float(ref.shape[1])
    return emd_ref64(ref, smp, True) / n, emd_ref64(ref, ref, True) / n, emd_ref64(smp, smp, True) / n


def stacked_1nn(M_rr, M_rs, M_ss):
    """The stacked matrix of the 1-NN two-sample test, diagonal at +inf."""
    D = torch.cat([torch.cat([M_rr, M_rs], 1), torch.cat([M_rs.t(), M_ss], 1)], 0).clone()
    D.fill_diagonal_(math.inf)
    return D
