"""Host: the plain dispatch rule of the bf16 GEMM (ldt_amd/csrc/gemm_bf16.hip, ldt_gemm_decide with no LN folding) against a restatement
written from its description, not from the C++.  ldt_gemm_route launches nothing: no GPU.

The rule.  K must be a multiple of 64, else no kernel takes the problem.  A launch may fill `lim` workgroups: max_wgs when 0 < max_wgs < 256,
else the 256 CUs.  The problem is big when its 256 x 256 tiles, ceil(M / 256) x ceil(N / 256) of them, fill at least 5/8 of `lim` and N > 128.
A problem that is not big goes to the mid-size tile kernels when their own rule (tests/test_gemm_mid_route_host.py, mid_tile) takes it.  A big
one with whole 256 x 256 tiles (M and N multiples of 256) and K >= 128 runs a 256-tile kernel.  Everything else runs the v1 kernel on the
largest of its three tiles that still gives every CU two workgroups (512 tiles): 128 x 128, then 128 x 64, else 64 x 64."""
import itertools

import pytest

from test_gemm_mid_route_host import EPIS, CANDIDATES, ceil_div, mid_tile

CUS = 256
V1_FORMS = ((128, 128), (128, 64), (64, 64))
MS = (64, 77, 100, 128, 130, 1000, 1024, 1960, 2048, 3000, 4096, 5000, 8192, 10496, 16384)
NS = (64, 128, 132, 192, 256, 768, 840, 1024, 1720, 2304, 3072, 4096)
KS = (64, 72, 128, 256, 320, 1024, 2048)
GRID = list(itertools.product(EPIS, MS, NS, KS, (0, 128)))


def expected(epi, M, N, K, max_wgs):
    """-> (family, BM, BN) with family in none / 256 / mid / v1"""
    if K % 64:
        return ("none", 0, 0)
    lim = max_wgs if 0 < max_wgs < CUS else CUS
    big = ceil_div(M, 256) * ceil_div(N, 256) * 8 >= 5 * lim and N > 128
    if not big:
        tile = mid_tile(epi, M, N, K, 0)
        if tile:
            return ("mid",) + tile
    if big and K >= 128 and M % 256 == 0 and N % 256 == 0:
        return ("256", 256, 256)
    for bm, bn in V1_FORMS[:2]:
        if ceil_div(M, bm) * ceil_div(N, bn) >= 2 * CUS:
            return ("v1", bm, bn)
    return ("v1",) + V1_FORMS[2]


@pytest.fixture(scope="module")
def route():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib, ops
    epi = dict(F32=_lib.EPI_F32, BF16=_lib.EPI_BF16, GELU=_lib.EPI_GELU_BF16, RELU=_lib.EPI_RELU_BF16, RESID=_lib.EPI_RESID_F32)
    family = {"none": "none", "256-one-tile": "256", "256-multi-tile": "256", "mid": "mid", "v1": "v1"}

    def plain_route(e, M, N, K, max_wgs):
        r = ops.gemm_route(epi[e], M, N, K, max_wgs=max_wgs)
        return (family[r.family], r.bm, r.bn), r.tiles_per_wg
    return plain_route


def test_grid_is_the_one_the_rule_was_checked_on():
    assert len(GRID) == 12600


def test_plain_rule_matches_the_restatement(route):
    reached = set()
    for e, M, N, K, max_wgs in GRID:
        want = expected(e, M, N, K, max_wgs)
        got, tiles_per_wg = route(e, M, N, K, max_wgs)
        assert got == want, (e, M, N, K, max_wgs, got, want)
        if want[0] in ("mid", "v1"):
            assert tiles_per_wg == 1, (e, M, N, K, max_wgs, tiles_per_wg)
        reached.add(want)
    # every family, and every tile of the v1 and mid-size families, is reached
    assert reached >= {("v1",) + f for f in V1_FORMS} | {("mid",) + c for c in CANDIDATES} | {("256", 256, 256), ("none", 0, 0)}, reached
