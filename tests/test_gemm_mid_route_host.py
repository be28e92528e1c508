"""Host: the shape rule of the mid-size tile kernels (ldt_amd/csrc/gemm_mid.hip, mid_form_for) against an independent restatement written
from its description, not from the C++.  ldt_gemm_route launches nothing: no GPU.

The rule.  The family takes the F32 / BF16 / GELU / RESID epilogues with K a multiple of 64, N a multiple of 64, M >= 64 and 16-byte output
rows.  Candidate tiles, in this order: 128 x 256, 128 x 192, 128 x 128, 64 x 128, 64 x 64.  A candidate is admitted when N is a multiple of
its width (192: bf16 outputs only) and its ceil(M / BM) x (N / BN) workgroups number 48 .. 2 x 256 (at most two rounds on the 256 CUs).  Its
cost is rounds x (BM + BN) with rounds = ceil(workgroups / 256); the first candidate of least cost wins.  LN-folded forms (statistics per
32 columns): the producer (RESID) runs 128-column tiles only; the consumers (BF16 / GELU) 128-row tiles only, with at most 32 statistics
parts (K <= 1024) and at least ring depth + 2 = 5 K-tiles.  In front of the rule the dispatch keeps a plain problem whose 256 x 256 tiles
fill 5/8 of the CUs (and N > 128) for the persistent kernel, and admits a folded one only with M a multiple of 128 and K >= 128."""
import itertools

import pytest

EPIS = ("F32", "BF16", "GELU", "RELU", "RESID")
CANDIDATES = ((128, 256), (128, 192), (128, 128), (64, 128), (64, 64))
CUS = 256


def ceil_div(a, b):
    return -(-a // b)


def mid_tile(epi, M, N, K, fold):
    """-> (BM, BN) of the form the rule picks, or None"""
    if epi == "RELU" or K % 64 or N % 64 or M < 64:
        return None
    bf16_out = epi in ("BF16", "GELU")
    if fold:
        if epi not in ("RESID", "BF16", "GELU"):
            return None
        if bf16_out and (K // 32 > 32 or K // 64 < 5):
            return None
    best = None
    for bm, bn in CANDIDATES:
        if N % bn or (bn == 192 and not bf16_out):
            continue
        if fold and ((epi == "RESID" and bn != 128) or (bf16_out and bm != 128)):
            continue
        wgs = ceil_div(M, bm) * (N // bn)
        if not 48 <= wgs <= 2 * CUS:
            continue
        cost = ceil_div(wgs, CUS) * (bm + bn)
        if best is None or cost < best[0]:
            best = (cost, bm, bn)
    return best and best[1:]


def expected(epi, M, N, K, fold):
    """-> (BM, BN) when the dispatch hands the problem to the mid-size tile kernels, else None"""
    if K % 64:
        return None
    if fold:
        return mid_tile(epi, M, N, K, fold) if M % 128 == 0 and K >= 128 else None
    if ceil_div(M, 256) * ceil_div(N, 256) * 8 >= CUS * 5 and N > 128:
        return None
    return mid_tile(epi, M, N, K, fold)


# what tests/test_gpu_kernel_exact.py::test_route_table pins for this family
PINNED = [(e, 2048, 4096, K, 0, (128, 256)) for e in ("F32", "BF16", "GELU", "RESID") for K in (64, 128, 192, 256)]
PINNED += [(e, 2048, 3072, K, 0, (128, 192)) for e in ("BF16", "GELU") for K in (64, 128, 192, 256)]
PINNED += [(e, 1024, 4096, K, 0, (128, 128)) for e in ("F32", "BF16", "GELU", "RESID") for K in (64, 128, 192, 256)]
PINNED += [("F32", 1960, 4096, 320, 0, (128, 256)), ("GELU", 1990, 3072, 320, 0, (128, 192)), ("RESID", 1000, 2304, 320, 0, (128, 128)),
           ("RESID", 2048, 1024, 320, 0, (64, 128)), ("BF16", 2000, 1024, 192, 0, (64, 128)), ("RESID", 1024, 1024, 448, 0, (64, 64)),
           ("F32", 1000, 1024, 704, 0, (64, 64)), ("RELU", 2048, 4096, 128, 0, None), ("BF16", 8192, 1024, 1024, 0, (128, 256)),
           ("RESID", 2048, 1024, 512, 32, (64, 128)), ("RESID", 4096, 1024, 512, 32, (128, 128)), ("BF16", 2048, 3072, 1024, 32, (128, 192)),
           ("GELU", 2048, 4096, 1024, 32, (128, 256)), ("BF16", 1024, 1024, 1024, 32, (128, 128)), ("RELU", 2048, 1024, 512, 32, None)]

GRID = list(itertools.product(EPIS, (64, 100, 128, 1000, 1024, 1960, 2048, 3000, 4096, 8192), (64, 128, 192, 256, 768, 1024, 2304, 3072, 4096),
                              (64, 128, 256, 320, 1024, 2048), (0, 32)))


@pytest.fixture(scope="module")
def route():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib, ops
    epi = dict(F32=_lib.EPI_F32, BF16=_lib.EPI_BF16, GELU=_lib.EPI_GELU_BF16, RELU=_lib.EPI_RELU_BF16, RESID=_lib.EPI_RESID_F32)

    def mid_route(e, M, N, K, fold):
        r = ops.gemm_route(epi[e], M, N, K, fold=fold)
        return (r.bm, r.bn) if r.family == "mid" else None
    return mid_route


def test_restatement_reproduces_the_pinned_table():
    for e, M, N, K, fold, tile in PINNED:
        assert expected(e, M, N, K, fold) == tile, (e, M, N, K, fold)


def test_rule_matches_the_restatement(route):
    points = [p[:5] for p in PINNED] + GRID
    taken = set()
    for e, M, N, K, fold in points:
        want = expected(e, M, N, K, fold)
        assert route(e, M, N, K, fold) == want, (e, M, N, K, fold, want)
        if want:
            taken.add((fold,) + want)
    # the points reach every form the rule can pick: five plain tiles, two producer tiles, three consumer tiles
    assert taken == {(0,) + c for c in CANDIDATES} | {(32, 128, 128), (32, 64, 128), (32, 128, 256), (32, 128, 192)}, taken


def test_folded_route_is_a_mid_form_or_nothing(route):
    import __graft_entry__  # noqa: F401
    from ldt_amd import _lib, ops
    for M, N, K in ((2048, 1024, 512), (1024, 1024, 64), (2048, 4096, 2048), (192, 1024, 512)):
        for e in (_lib.EPI_RESID_F32, _lib.EPI_BF16, _lib.EPI_GELU_BF16):
            assert ops.gemm_route(e, M, N, K, fold=32).family in ("mid", "none"), (e, M, N, K)
