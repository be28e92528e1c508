"""Entry checks of the three bf16 GEMM entries (ldt_gemm_bf16, ldt_gemm_resid_lnstats, ldt_gemm_lnfold; csrc/api.hip and the launchers of
csrc/gemm_bf16.hip): every refusal comes back as a status code with a message that names the entry or the launcher.  Every call here breaks
at least one rule, so nothing is launched and no GPU is needed; the pointers are made-up integers that are only ever compared and masked.

The cases of each table stand in the order of the checks.  A folded call passes two sets of checks: the entry's own (null pointers, a
stats_parts that is neither granule), then the folded launcher's, whose messages begin "gemm_lnfold"."""
import pytest

EARG, ESHAPE, EALIGN = -1, -2, -3
F32, BF16, GELU, RELU, RESID = range(5)
P = 1 << 20                     # a 16-byte aligned "pointer"
Q8 = P + 8                      # 8-byte aligned only

# 256 x 256 x 64: the smallest sound plain problem (it would run the v1 kernel)
GEMM = dict(epilogue=BF16, X=P, ldx=64, W=P, ldw=64, bias=P, out=P, ldo=256, resid=None, ldr=0, skip=None, ldskip=0, gate=None,
            gate_sample_stride=0, rows_per_sample=0, step_ptr=None, gate_step_stride=0, M=256, N=256, K=64)
RES = dict(epilogue=RESID, resid=P, ldr=256)
GEMM_CASES = [
    (dict(X=None), EARG), (dict(W=None), EARG), (dict(out=None), EARG),
    (dict(M=0), ESHAPE), (dict(N=0), ESHAPE), (dict(K=0), ESHAPE), (dict(M=-256), ESHAPE),
    (dict(K=72, ldx=72, ldw=72), ESHAPE), (dict(K=32), ESHAPE),
    (dict(ldx=68), EALIGN), (dict(ldw=68), EALIGN), (dict(X=Q8), EALIGN), (dict(W=Q8), EALIGN),
    (dict(ldx=56), ESHAPE), (dict(ldw=56), ESHAPE),
    (dict(ldo=258), EALIGN), (dict(out=Q8), EALIGN),
    (dict(epilogue=RESID), EALIGN), (dict(RES, resid=Q8), EALIGN), (dict(RES, ldr=258), EALIGN),
    (dict(RES, gate=P), EARG), (dict(RES, gate=Q8, rows_per_sample=32), EARG), (dict(RES, gate=P, rows_per_sample=32, gate_sample_stride=258), EARG),
    (dict(RES, gate=P, rows_per_sample=32, gate_step_stride=258), EARG),
    (dict(bias=Q8), EALIGN), (dict(RES, bias=Q8), EALIGN),
    (dict(epilogue=7), EARG), (dict(epilogue=-1), EARG),
    # two rules broken: the earlier check answers
    (dict(X=None, M=0), EARG), (dict(M=0, K=72), ESHAPE), (dict(K=72, X=Q8), ESHAPE), (dict(ldx=68, ldw=56), EALIGN), (dict(ldx=56, ldo=258), ESHAPE),
    (dict(out=Q8, epilogue=RESID), EALIGN), (dict(RES, gate=P, bias=Q8), EARG), (dict(epilogue=7, bias=Q8), EALIGN),
]

# producer: 256 x 256 x 256 with statistics per 256 columns (one part), and 2048 x 1024 x 512 with statistics per 32 columns (32 parts)
PROD = dict(X=P, ldx=256, W=P, ldw=256, bias=P, out=P, ldo=256, gate=None, gate_sample_stride=0, rows_per_sample=0, ln_scale=P, xs=P, ldxs=256,
            stats_out=P, step_ptr=None, gate_step_stride=0, ln_step_stride=0, M=256, N=256, K=256, stats_parts=1)
PROD32 = dict(PROD, ldx=512, ldw=512, ldo=1024, ldxs=1024, M=2048, N=1024, K=512, stats_parts=32)
PROD_ENTRY = [          # answered by ldt_gemm_resid_lnstats itself
    (PROD, dict(X=None), EARG), (PROD, dict(W=None), EARG), (PROD, dict(out=None), EARG), (PROD, dict(xs=None), EARG), (PROD, dict(ln_scale=None), EARG),
    (PROD, dict(stats_out=None), EARG),
    (PROD, dict(stats_parts=2), EARG), (PROD, dict(stats_parts=0), EARG), (PROD32, dict(stats_parts=16), EARG), (PROD, dict(xs=None, stats_parts=2), EARG),
]
PROD_LAUNCH = [         # answered by the folded launcher
    (PROD32, dict(M=2112), ESHAPE), (PROD32, dict(M=0), ESHAPE), (PROD32, dict(N=1056, stats_parts=33), ESHAPE), (PROD32, dict(K=64), ESHAPE),
    (PROD32, dict(K=160), ESHAPE),
    (PROD, dict(M=384), ESHAPE), (PROD, dict(M=0), ESHAPE), (PROD, dict(K=128), ESHAPE), (PROD, dict(K=288, ldx=288, ldw=288), ESHAPE),
    (PROD, dict(ldx=260), EALIGN), (PROD, dict(ldw=260), EALIGN), (PROD, dict(ldx=192), EALIGN), (PROD, dict(ldw=192), EALIGN),
    (PROD, dict(ldo=260), EALIGN), (PROD, dict(X=Q8), EALIGN), (PROD, dict(W=Q8), EALIGN), (PROD, dict(out=Q8), EALIGN), (PROD32, dict(ldx=448), EALIGN),
    (PROD, dict(gate=P), EARG), (PROD, dict(gate=P, rows_per_sample=32, gate_sample_stride=258), EARG), (PROD, dict(bias=Q8), EALIGN),
    (PROD, dict(xs=Q8), EARG), (PROD, dict(ldxs=128), EARG), (PROD, dict(ldxs=258), EARG), (PROD, dict(ln_scale=Q8), EARG), (PROD, dict(stats_out=Q8), EARG),
    (PROD, dict(ln_step_stride=258), EARG), (PROD32, dict(xs=Q8), EARG),
    (PROD32, dict(M=128, N=128, K=128, stats_parts=4), ESHAPE),       # a sound call that the mid-size tile kernel has no producer form for
    # two rules broken: the earlier check answers
    (PROD, dict(M=384, ldx=260), ESHAPE), (PROD, dict(ldx=260, gate=P), EALIGN), (PROD, dict(gate=P, xs=Q8), EARG), (PROD, dict(bias=Q8, xs=Q8), EALIGN),
]

# consumer: 256 x 256 x 256 with one statistics part, and 2048 x 1024 x 1024 with 32 parts (statistics per 32 columns)
CONS = dict(epilogue=BF16, Xs=P, ldx=256, W=P, ldw=256, stats_in=P, fold_S=P, fold_C=P, out=P, ldo=256, step_ptr=None, fold_step_stride=0,
            M=256, N=256, K=256, stats_parts=1)
CONS32 = dict(CONS, ldx=1024, ldw=1024, ldo=1024, M=2048, N=1024, K=1024, stats_parts=32)
CONS_ENTRY = [          # answered by ldt_gemm_lnfold itself
    (CONS, dict(Xs=None), EARG), (CONS, dict(W=None), EARG), (CONS, dict(out=None), EARG), (CONS, dict(stats_in=None), EARG), (CONS, dict(fold_S=None), EARG),
    (CONS, dict(fold_C=None), EARG),
    (CONS, dict(stats_parts=2), EARG), (CONS, dict(stats_parts=0), EARG), (CONS32, dict(stats_parts=8), EARG), (CONS, dict(fold_S=None, stats_parts=2), EARG),
]
CONS_LAUNCH = [         # answered by the folded launcher
    (CONS32, dict(M=2112), ESHAPE), (CONS32, dict(N=1056), ESHAPE), (CONS32, dict(K=160, stats_parts=5), ESHAPE), (CONS32, dict(K=96, stats_parts=3), ESHAPE),
    (CONS, dict(M=384), ESHAPE), (CONS, dict(N=384), ESHAPE), (CONS, dict(M=0), ESHAPE),
    (CONS, dict(ldx=260), EALIGN), (CONS, dict(ldw=192), EALIGN), (CONS, dict(ldo=260), EALIGN), (CONS, dict(Xs=Q8), EALIGN), (CONS, dict(out=Q8), EALIGN),
    (CONS, dict(epilogue=RESID), EALIGN),                             # the producer's epilogue: its residual operand is missing
    (CONS, dict(epilogue=RELU), EARG), (CONS, dict(epilogue=F32), EARG), (CONS32, dict(epilogue=RELU), EARG), (CONS, dict(epilogue=7), EARG),
    (CONS, dict(fold_S=Q8), EARG), (CONS, dict(fold_C=Q8), EARG), (CONS, dict(stats_in=Q8), EARG), (CONS, dict(fold_step_stride=258), EARG),
    (CONS32, dict(fold_S=Q8), EARG),
    (CONS32, dict(K=2048, ldx=2048, ldw=2048, stats_parts=64), ESHAPE),       # statistics per 32 columns: at most 32 parts
    (CONS, dict(K=2048, ldx=2048, ldw=2048, stats_parts=8), EARG),            # statistics per 256 columns: at most 4 parts
    (CONS32, dict(M=128, N=128, stats_parts=32), ESHAPE),             # a sound call that the mid-size tile kernel has no consumer form for
    # two rules broken: the earlier check answers
    (CONS, dict(M=384, ldx=260), ESHAPE), (CONS, dict(ldx=260, epilogue=RELU), EALIGN), (CONS, dict(epilogue=RELU, fold_S=Q8), EARG),
    (CONS, dict(fold_S=Q8, K=2048, ldx=2048, ldw=2048, stats_parts=8), EARG),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    lib = _lib.lib()
    assert lib.ldt_abi_version() == 26
    return lib


def refused(lib, entry, base, broken, status, prefix):
    assert broken and all(k in base for k in broken), broken          # a call that broke nothing would launch on made-up pointers
    got = getattr(lib, entry)(*{**base, **broken}.values(), None)
    msg = lib.ldt_last_error()
    assert got == status and msg.startswith(prefix), (entry, broken, "status %d, expected %d" % (got, status), msg)
    return msg


def test_gemm_bf16_refusals(lib):
    for broken, status in GEMM_CASES:
        refused(lib, "ldt_gemm_bf16", GEMM, broken, status, b"gemm: ")
    # same code, so the message tells which check answered
    assert b"empty problem" in refused(lib, "ldt_gemm_bf16", GEMM, dict(M=0, K=72), ESHAPE, b"gemm: ")
    assert b"multiple of 64" in refused(lib, "ldt_gemm_bf16", GEMM, dict(K=72, ldx=56), ESHAPE, b"gemm: ")
    assert b"resid" in refused(lib, "ldt_gemm_bf16", GEMM, dict(epilogue=RESID, bias=Q8), EALIGN, b"gemm: ")
    assert b"bias" in refused(lib, "ldt_gemm_bf16", GEMM, dict(bias=Q8), EALIGN, b"gemm: ")
    assert b"unknown epilogue 7" in refused(lib, "ldt_gemm_bf16", GEMM, dict(epilogue=7), EARG, b"gemm: ")


def test_gemm_resid_lnstats_refusals(lib):
    for base, broken, status in PROD_ENTRY:
        refused(lib, "ldt_gemm_resid_lnstats", base, broken, status, b"gemm_resid_lnstats: ")
    for base, broken, status in PROD_LAUNCH:
        refused(lib, "ldt_gemm_resid_lnstats", base, broken, status, b"gemm_lnfold")
    assert b"null pointer" in refused(lib, "ldt_gemm_resid_lnstats", PROD, dict(xs=None), EARG, b"gemm_resid_lnstats: ")
    assert b"stats_parts=2" in refused(lib, "ldt_gemm_resid_lnstats", PROD, dict(stats_parts=2), EARG, b"gemm_resid_lnstats: ")
    assert b"multiple of 128" in refused(lib, "ldt_gemm_resid_lnstats", PROD32, dict(M=2112), ESHAPE, b"gemm_lnfold")
    assert b"multiples of 256" in refused(lib, "ldt_gemm_resid_lnstats", PROD, dict(M=384), ESHAPE, b"gemm_lnfold: ")
    assert b"producer needs xs" in refused(lib, "ldt_gemm_resid_lnstats", PROD, dict(ldxs=128), EARG, b"gemm_lnfold: ")
    assert b"as a producer" in refused(lib, "ldt_gemm_resid_lnstats", PROD32, dict(M=128, N=128, K=128, stats_parts=4), ESHAPE, b"gemm_lnfold: ")


def test_gemm_lnfold_refusals(lib):
    for base, broken, status in CONS_ENTRY:
        refused(lib, "ldt_gemm_lnfold", base, broken, status, b"gemm_lnfold: ")
    for base, broken, status in CONS_LAUNCH:
        refused(lib, "ldt_gemm_lnfold", base, broken, status, b"gemm_lnfold")
    assert b"null pointer" in refused(lib, "ldt_gemm_lnfold", CONS, dict(fold_S=None), EARG, b"gemm_lnfold: ")
    assert b"stats_parts=2" in refused(lib, "ldt_gemm_lnfold", CONS, dict(stats_parts=2), EARG, b"gemm_lnfold: ")
    assert b"epilogue 3 has no folded form" in refused(lib, "ldt_gemm_lnfold", CONS, dict(epilogue=RELU), EARG, b"gemm_lnfold: ")
    assert b"consumer needs stats_in" in refused(lib, "ldt_gemm_lnfold", CONS, dict(fold_S=Q8), EARG, b"gemm_lnfold: ")
    assert b"K=2048 > 1024" in refused(lib, "ldt_gemm_lnfold", CONS32, dict(K=2048, ldx=2048, ldw=2048, stats_parts=64), ESHAPE, b"gemm_lnfold")
    assert b"K=2048" in refused(lib, "ldt_gemm_lnfold", CONS, dict(K=2048, ldx=2048, ldw=2048, stats_parts=8), EARG, b"gemm_lnfold: ")
    assert b"as a consumer" in refused(lib, "ldt_gemm_lnfold", CONS32, dict(M=128, N=128, stats_parts=32), ESHAPE, b"gemm_lnfold: ")
