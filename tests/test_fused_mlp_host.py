"""Entry checks of the fused narrow-block kernels (csrc/fused_mlp.hip behind ldt_ln_mlp_resid, ldt_ln_mlp_resid_next and ldt_ln_linear):
every refusal comes back as a status code with a message that names the entry.  Every call here breaks at least one rule, so nothing is
launched and no GPU is needed; the pointers are made-up integers that are only ever compared and masked.

The order of the checks is behaviour (a caller sees the first rule it broke), so where two rules are broken the winner is asserted.
The three places that state the LayerNorm-source rules do not agree on the code, and that is pinned as it stands: the MLP's own LayerNorm
and ldt_ln_linear answer LDT_EARG for a missing half of a pair or a bad per-sample stride and LDT_EALIGN for a misaligned vector (except
that ldt_ln_linear files a misaligned shift / scale under LDT_EARG), the chained projection answers LDT_EARG for everything."""
import pytest

EARG, ESHAPE, EALIGN = -1, -2, -3
P = 1 << 20                     # a 16-byte aligned "pointer"
Q8, Q4 = P + 8, P + 4           # 8-byte and 4-byte aligned only

MLP = dict(x=P, ldx=128, M=300, C=128, ln_w=P, ln_b=P, shift=None, scale=None, gate=None, mod_sample_stride=0, rows_per_sample=0,
           w_up=P, b_up=P, w_dn=P, b_dn=P, x_bf16=None, ldxb=0)
NEXT = dict(nx_ln_w=P, nx_ln_b=P, nx_shift=None, nx_scale=None, nx_mod_sample_stride=0, nx_rows_per_sample=0, nx_w=P, nx_bias=P,
            nx_N=128, nx_out=P, nx_ldo=128)
LIN = dict(x=P, ldx=128, M=300, C=128, ln_w=P, ln_b=P, shift=None, scale=None, mod_sample_stride=0, rows_per_sample=0,
           w=P, bias=P, N=128, out=P, ldo=128)
MOD = dict(ln_w=None, ln_b=None, shift=P, scale=P, mod_sample_stride=384, rows_per_sample=100)      # a sound AdaLN modulation
NX_MOD = {"nx_" + k: v for k, v in MOD.items()}

# (what is broken, expected status): the head that ldt_ln_mlp_resid and ldt_ln_mlp_resid_next share, in the order of the checks
MLP_HEAD = [
    (dict(x=None), EARG), (dict(w_up=None), EARG), (dict(b_up=None), EARG), (dict(w_dn=None), EARG), (dict(b_dn=None), EARG),
    (dict(M=0), ESHAPE), (dict(M=-5), ESHAPE),
    (dict(C=96), ESHAPE), (dict(C=256, ldx=256), ESHAPE), (dict(C=32), ESHAPE),
    (dict(ldx=64), EALIGN), (dict(ldx=130), EALIGN), (dict(C=64, ldx=32), EALIGN), (dict(x=Q8), EALIGN),
    (dict(ln_b=None), EARG), (dict(ln_w=None), EARG),
    (dict(shift=P), EARG), (dict(scale=P), EARG),
    (dict(MOD, rows_per_sample=0), EARG), (dict(MOD, rows_per_sample=-1), EARG), (dict(MOD, mod_sample_stride=386), EARG),
    (dict(gate=P), EARG), (dict(gate=P, rows_per_sample=100, mod_sample_stride=386), EARG),
    (dict(MOD, gate=P, rows_per_sample=0), EARG),
    (dict(w_up=Q8), EALIGN), (dict(w_dn=Q8), EALIGN), (dict(b_up=Q8), EALIGN), (dict(b_dn=Q8), EALIGN),
    (dict(ln_w=Q8), EALIGN), (dict(ln_b=Q8), EALIGN), (dict(MOD, shift=Q8), EALIGN), (dict(MOD, scale=Q8), EALIGN),
    (dict(MOD, gate=Q8), EALIGN), (dict(gate=Q4, rows_per_sample=100, mod_sample_stride=384), EALIGN),
    (dict(x_bf16=P, ldxb=64), EALIGN), (dict(x_bf16=P, ldxb=130), EALIGN), (dict(x_bf16=Q4, ldxb=128), EALIGN),
    (dict(C=64, ldx=64, x_bf16=P, ldxb=32), EALIGN),
    # two rules broken: the earlier check answers
    (dict(x=None, M=0), EARG), (dict(b_dn=None, C=96), EARG),
    (dict(M=0, x=Q8), ESHAPE), (dict(C=96, x=Q8), ESHAPE), (dict(C=96, ln_b=None), ESHAPE),
    (dict(ldx=130, ln_b=None), EALIGN), (dict(x=Q8, shift=P), EALIGN), (dict(x=Q8, gate=P), EALIGN),
    (dict(ln_b=None, w_up=Q8), EARG), (dict(ln_w=Q8, ln_b=None), EARG), (dict(shift=Q8), EARG), (dict(MOD, rows_per_sample=0, shift=Q8), EARG),
    (dict(gate=Q8), EARG), (dict(MOD, mod_sample_stride=386, b_dn=Q8), EARG), (dict(ln_b=None, x_bf16=P, ldxb=64), EARG),
]
# the chained projection of ldt_ln_mlp_resid_next: one code for every fault, answered after the MLP's own operands and before the mirror
MLP_NEXT = [
    (dict(nx_w=None), EARG), (dict(nx_out=None), EARG),
    (dict(nx_N=0), EARG), (dict(nx_N=-64), EARG), (dict(nx_N=100), EARG), (dict(nx_N=96, nx_ldo=96), EARG),
    (dict(nx_ldo=64), EARG), (dict(nx_ldo=132), EARG), (dict(nx_out=Q8), EARG),
    (dict(nx_w=Q8), EARG), (dict(nx_bias=Q8), EARG),
    (dict(nx_ln_b=None), EARG), (dict(nx_ln_w=None), EARG), (dict(nx_shift=P), EARG), (dict(nx_scale=P), EARG),
    (dict(NX_MOD, nx_rows_per_sample=0), EARG), (dict(NX_MOD, nx_mod_sample_stride=386), EARG),
    (dict(nx_ln_w=Q8), EARG), (dict(nx_ln_b=Q8), EARG), (dict(NX_MOD, nx_shift=Q8), EARG), (dict(NX_MOD, nx_scale=Q8), EARG),
    # against the MLP's own rules and the mirror
    (dict(nx_w=None, M=0), EARG), (dict(nx_N=100, M=0), ESHAPE), (dict(nx_N=100, x=Q8), EALIGN), (dict(nx_N=100, w_up=Q8), EALIGN),
    (dict(nx_ln_w=Q8, ln_w=Q8), EALIGN), (dict(nx_N=100, ln_b=None), EARG),
    (dict(nx_N=100, x_bf16=P, ldxb=64), EARG), (dict(nx_ln_w=Q8, x_bf16=Q4, ldxb=128), EARG), (dict(NX_MOD, nx_shift=Q8, x_bf16=P, ldxb=130), EARG),
]
LINEAR = [
    (dict(x=None), EARG), (dict(w=None), EARG), (dict(out=None), EARG),
    (dict(M=0), ESHAPE), (dict(M=-5), ESHAPE), (dict(C=96), ESHAPE), (dict(C=256, ldx=256), ESHAPE),
    (dict(N=0), ESHAPE), (dict(N=-64), ESHAPE), (dict(N=100), ESHAPE), (dict(N=96, ldo=96), ESHAPE),
    (dict(ldx=64), EALIGN), (dict(ldx=130), EALIGN), (dict(C=64, ldx=32), EALIGN), (dict(x=Q8), EALIGN),
    (dict(ldo=64), EALIGN), (dict(ldo=132), EALIGN), (dict(out=Q8), EALIGN), (dict(w=Q8), EALIGN), (dict(bias=Q8), EALIGN),
    (dict(ln_b=None), EARG), (dict(ln_w=None), EARG), (dict(shift=P), EARG), (dict(scale=P), EARG),
    (dict(MOD, rows_per_sample=0), EARG), (dict(MOD, rows_per_sample=-1), EARG), (dict(MOD, mod_sample_stride=386), EARG),
    (dict(MOD, shift=Q8), EARG), (dict(MOD, scale=Q8), EARG),
    (dict(ln_w=Q8), EALIGN), (dict(ln_b=Q8), EALIGN),
    # two rules broken: the earlier check answers
    (dict(out=None, M=0), EARG), (dict(M=0, N=100), ESHAPE), (dict(C=96, x=Q8), ESHAPE), (dict(N=100, x=Q8), ESHAPE), (dict(N=100, ln_b=None), ESHAPE),
    (dict(x=Q8, ln_b=None), EALIGN), (dict(bias=Q8, shift=P), EALIGN), (dict(MOD, ldo=132, rows_per_sample=0), EALIGN),
    (dict(ln_w=Q8, ln_b=None), EARG), (dict(ln_w=Q8, scale=P), EARG),
    (dict(shift=P, scale=P, mod_sample_stride=384, rows_per_sample=0, ln_w=Q8), EARG), (dict(shift=Q8, scale=P, mod_sample_stride=384, rows_per_sample=100, ln_w=Q8), EARG),
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


def test_ln_mlp_resid_refusals(lib):
    for broken, status in MLP_HEAD:
        refused(lib, "ldt_ln_mlp_resid", MLP, broken, status, b"ln_mlp: ")
        refused(lib, "ldt_ln_mlp_resid_next", {**MLP, **NEXT}, broken, status, b"ln_mlp")
    # same code, so the message tells which check answered: the row count is judged before the channel count
    assert b"row count" in refused(lib, "ldt_ln_mlp_resid", MLP, dict(M=0, C=96), ESHAPE, b"ln_mlp: ")
    assert b"64 or 128 channels" in refused(lib, "ldt_ln_mlp_resid", MLP, dict(C=96), ESHAPE, b"ln_mlp: ")


def test_ln_mlp_resid_next_refusals(lib):
    for broken, status in MLP_NEXT:
        refused(lib, "ldt_ln_mlp_resid_next", {**MLP, **NEXT}, broken, status, b"ln_mlp")
    assert b"follow-on" in refused(lib, "ldt_ln_mlp_resid_next", {**MLP, **NEXT}, dict(nx_N=100), EARG, b"ln_mlp: ")


def test_ln_linear_refusals(lib):
    for broken, status in LINEAR:
        refused(lib, "ldt_ln_linear", LIN, broken, status, b"ln_linear: ")
    assert b"row count" in refused(lib, "ldt_ln_linear", LIN, dict(M=0, C=96), ESHAPE, b"ln_linear: ")
    assert b"N=100" in refused(lib, "ldt_ln_linear", LIN, dict(N=100, ldo=64), ESHAPE, b"ln_linear: ")
