"""Host: the dispatch rule of the fp32 linear (ldt_sgemm_decide in ldt_amd/csrc/sgemm.hip, queried through ldt_sgemm_route) against a
restatement written from the description in include/ldt_hip.h, not from the C++.  The query launches nothing and touches no device: no GPU.

The rule.  A problem with M, N or K below 1 has no kernel.  "A and W rows load 16 bytes" means K, lda and ldb are multiples of 4 and neither
A nor W is misaligned.  The forms are tried in this order and the first that takes the problem runs it:
  small-N streaming <4> / <8>   M >= 8192, N <= 8 (<4> up to 4), A and W rows load 16 bytes
  small-K streaming <4> / <8>   M >= 8192, K <= 8 (<4> up to 4), N in {32, 64, 128, 256, 512, 1024}, ldc a multiple of 4, C and bias aligned
  MFMA 32 x 128                 M <= 48, K >= 8, M N >= 4096, A and W rows load 16 bytes
  MFMA 128 x 128                the same with M > 48, while ceil(M / 128) < 65536
  scalar-FMA kernel             everything else while ceil(M / 64) < 65536
LDT_SGEMM_VALU (set) takes the two MFMA forms out, LDT_SGEMM_SKINNY=0 the four streaming ones; both are read once per process."""
import itertools
import os
import subprocess
import sys

import pytest

import sgemm_checks as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT_MAX_M = 65535 * 64                 # the scalar kernel's last M: grid.y = ceil(M / 64) < 65536
MFMA_MAX_M = 65535 * 128
MS = (0, 1, 47, 48, 49, 63, 64, 4095, 4096, 8191, 8192, 8200, 30000, NT_MAX_M, NT_MAX_M + 1, MFMA_MAX_M, MFMA_MAX_M + 1)
NS = (1, 4, 5, 8, 9, 28, 32, 64, 65, 96, 1024, 1028)
KS = (1, 3, 4, 7, 8, 9, 12, 16, 20)
PADS = list(itertools.product((0, 4, 1), (0, 2), (0, 4, 3)))       # lda - K, ldb - K, ldc - N
GRID = list(itertools.product(MS, NS, KS, PADS, range(16)))


def expected(M, N, K, lda, ldb, ldc, mis, valu=False, skinny=True):
    if min(M, N, K) < 1:
        return 0
    rows16 = K % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and not mis & 1 and not mis & 2
    if skinny and M >= 8192:
        if N <= 8 and rows16:
            return 4 if N <= 4 else 5
        if K <= 8 and N in (32, 64, 128, 256, 512, 1024) and ldc % 4 == 0 and not mis & 4 and not mis & 8:
            return 6 if K <= 4 else 7
    if not valu and rows16 and K >= 8 and M * N >= 4096:
        if M <= 48:
            return 3
        if -(-M // 128) < 65536:
            return 2
    return 1 if -(-M // 64) < 65536 else 0


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import ops
    return ops


def test_grid_is_the_one_the_rule_was_checked_on():
    assert len(GRID) == 17 * 12 * 9 * 18 * 16
    assert {48, 49, 8191, 8192} <= set(MS) and {4, 7, 8, 9} <= set(KS) and {8, 9, 28, 32, 96, 1024, 1028} <= set(NS)
    assert 63 * 65 == 4095 and 64 * 64 == 4096 and {63, 64} <= set(MS) and {64, 65} <= set(NS)       # M N on either side of 4096
    assert NT_MAX_M + 1 in MS


def test_rule_matches_the_restatement(ops):
    reached = set()
    for M, N, K, (pa, pb, pc), mis in GRID:
        want = expected(M, N, K, K + pa, K + pb, N + pc, mis)
        got = ops.sgemm_route_shape(M, N, K, K + pa, K + pb, N + pc, mis)
        assert got == want, (M, N, K, pa, pb, pc, mis, got, want)
        reached.add(want)
    assert reached == set(range(8)), reached


def test_every_case_of_the_table_takes_the_route_it_names(ops):
    """the labels of SGEMM_CASES (and of the older tests' shapes) are the launcher's own answers, so none can go stale"""
    assert {c.route for c in sc.SGEMM_CASES} == set(range(1, 8))
    assert len({c.name for c in sc.SGEMM_CASES}) == len(sc.SGEMM_CASES)
    for c in sc.SGEMM_CASES:
        mis = {"dense": 0, "a+4": 1}[c.view]
        assert ops.sgemm_route_shape(c.M, c.N, c.K, misaligned=mis) == c.route == expected(c.M, c.N, c.K, c.K, c.K, c.N, mis), c
    for (M, N, K), route in sc.LEGACY_ROUTES.items():
        assert ops.sgemm_route_shape(M, N, K) == route == expected(M, N, K, K, K, N, 0), (M, N, K)
    for name in sc.REPRESENTATIVES + sc.PAST_THE_CAP:
        assert name in sc.CASE
    assert sorted(sc.CASE[n].route for n in sc.REPRESENTATIVES) == list(range(1, 8))
    # past the cap: the rows of one pass of the grid (at the MI355X's 256 CUs) end before M, for all four streaming kernels
    assert sorted({sc.CASE[n].route for n in sc.PAST_THE_CAP}) == [4, 5, 6, 7]
    for n in sc.PAST_THE_CAP:
        c = sc.CASE[n]
        assert sc.rows_per_pass(c.route, c.N) < c.M, c
    c = sc.CASE["smallk4-20000x1024x3"]
    assert 2 * sc.rows_per_pass(c.route, c.N) < c.M < 3 * sc.rows_per_pass(c.route, c.N)
    # the two pairs sit on either side of a threshold
    assert (sc.CASE["pair-8191x128x3"].route, sc.CASE["pair-8192x128x3"].route) == (1, 6)
    assert (sc.CASE["pair-48x200x64"].route, sc.CASE["pair-49x200x64"].route) == (3, 2)


CHILD = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
L.ldt_sgemm_route.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_int64] * 3 + [ctypes.c_int32]
shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[2:]]
print(" ".join(str(L.ldt_sgemm_route(M, N, K, K, K, N, 0)) for M, N, K in shapes))
"""
SWITCH_SHAPES = ((130, 300, 256), (19, 2085, 512), (8200, 4, 128), (8193, 8, 64), (8201, 64, 4), (8197, 32, 7), (8192, 128, 8), (5, 64, 3))


@pytest.mark.parametrize("env,valu,skinny", [({}, False, True), ({"LDT_SGEMM_VALU": "1"}, True, True), ({"LDT_SGEMM_VALU": "0"}, True, True),
                                             ({"LDT_SGEMM_SKINNY": "0"}, False, False), ({"LDT_SGEMM_SKINNY": "1"}, False, True),
                                             ({"LDT_SGEMM_VALU": "1", "LDT_SGEMM_SKINNY": "0"}, True, False)])
def test_environment_switches_in_a_fresh_process(ops, env, valu, skinny):
    """LDT_SGEMM_VALU counts when set (to anything), LDT_SGEMM_SKINNY when it reads 0; each process reads them once, so each runs in a child"""
    from ldt_amd import _lib
    e = {k: v for k, v in os.environ.items() if k not in ("LDT_SGEMM_VALU", "LDT_SGEMM_SKINNY")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH] + ["%dx%dx%d" % s for s in SWITCH_SHAPES], env=e, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in r.stdout.split()]
    want = [expected(M, N, K, K, K, N, 0, valu=valu, skinny=skinny) for M, N, K in SWITCH_SHAPES]
    assert got == want, (env, got, want)
    if not env:
        assert set(got) == set(range(1, 8))               # the shapes do reach every form when nothing is switched off


def test_wrapper_reads_strides_and_alignment_from_the_tensors(ops):
    import torch
    M, N, K = 130, 300, 256
    a, w, b = torch.zeros(M, K + 8), torch.zeros(N, K + 8), torch.zeros(N + 4)
    out = torch.zeros(M, N + 8)
    assert a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    assert ops.sgemm_route(a[:, 4:4 + K], w[:, 4:4 + K], b[:N], out[:, 4:4 + N]) == 2 == ops.sgemm_route_shape(M, N, K, K + 8, K + 8, N + 8)
    assert ops.sgemm_route(a[:, 1:1 + K], w[:, 4:4 + K], b[:N], out[:, 4:4 + N]) == 1 == ops.sgemm_route_shape(M, N, K, K + 8, K + 8, N + 8, 1)
    assert ops.sgemm_route(a[:, :K], w[:, 3:3 + K]) == 1 == ops.sgemm_route_shape(M, N, K, K + 8, K + 8, N, 2)
    big = torch.zeros(8192, 8)
    ws = torch.zeros(128, 8)
    o = torch.zeros(8192, 136)
    assert ops.sgemm_route(big[:, :3], ws[:, :3], b[:128], o[:, 4:132]) == 6
    assert ops.sgemm_route(big[:, :3], ws[:, :3], b[:128], o[:, 1:129]) == 1 == ops.sgemm_route_shape(8192, 128, 3, 8, 8, 136, 4)
    assert ops.sgemm_route(big[:, :3], ws[:, :3], b[1:129], o[:, 4:132]) == 1 == ops.sgemm_route_shape(8192, 128, 3, 8, 8, 136, 8)
    assert ops.sgemm_route(big[:, :3], ws[:, :3], None, o[:, 4:132]) == 6
