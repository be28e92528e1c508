"""CPU: the entry contract of the small ops (one C-ABI entry per op, in the file of its kernel): every entry called through ctypes with a
null pointer and with one bad argument per check that precedes the launch, and the status plus the exact ldt_last_error() text held as
literals.  Every call here returns before any HIP call, so no device is needed; the pointers are made-up addresses that nothing reads."""
import pytest

P = 4096                                          # a 16-byte aligned address that is never dereferenced
ODD = 4100                                        # 4-byte aligned only
F = 0.0                                           # a float argument
OK, EARG, ESHAPE, EALIGN = 0, -1, -2, -3

CASES = [
    # -- elementwise.hip
    ("ldt_cast_pad_bf16", (None, 8, P, 8, 2, 4, 8, None), EARG, "cast_pad: null pointer"),
    ("ldt_cast_pad_bf16", (P, 8, None, 8, 2, 4, 8, None), EARG, "cast_pad: null pointer"),
    ("ldt_cast_pad_bf16", (P, 8, P, 8, 2, 4, 6, None), ESHAPE, "cast_pad: bad shape rows=2 cols=4 cols_pad=6 ldd=8"),
    ("ldt_cast_pad_bf16", (P, 8, P, 6, 2, 4, 8, None), ESHAPE, "cast_pad: bad shape rows=2 cols=4 cols_pad=8 ldd=6"),
    ("ldt_cast_pad_bf16", (P, 8, ODD, 8, 2, 4, 8, None), EALIGN, "cast_pad: dst must be 8-byte aligned"),
    ("ldt_layernorm_modulate", (None, 8, P, 8, None, None, None, None, 0, 1, None, 0, 2, 8, None), EARG, "ln: null pointer"),
    ("ldt_layernorm_modulate", (P, 8, P, 8, None, None, None, None, 0, 1, None, 0, 0, 8, None), ESHAPE, "ln: empty problem"),
    ("ldt_layernorm_modulate", (P, 8, P, 8, None, None, P, None, 0, 1, None, 0, 2, 8, None), EARG, "ln: shift and scale go together"),
    ("ldt_layernorm_modulate", (P, 8, P, 8, P, None, None, None, 0, 1, None, 0, 2, 8, None), EARG, "ln: affine weight and bias go together"),
    ("ldt_layernorm_modulate", (P, 8, P, 8, None, None, P, P, 0, 0, None, 0, 2, 8, None), EARG, "ln: rows_per_sample must be > 0 with modulation"),
    ("ldt_sinusoid", (P, None, P, 2, 4, None), EARG, "sinusoid: null pointer"),
    ("ldt_sinusoid", (P, P, P, 0, 4, None), ESHAPE, "sinusoid: empty"),
    ("ldt_sinusoid", (P, P, P, 2, 0, None), ESHAPE, "sinusoid: empty"),
    # -- sgemm.hip
    ("ldt_sgemm", (P, 4, P, 4, None, P, 4, 0, 0, 0, 0, 4, 4, None), ESHAPE, "sgemm: empty problem"),
    ("ldt_sgemm", (None, 4, None, 4, None, None, 4, 0, 0, 0, 0, 4, 4, None), ESHAPE, "sgemm: empty problem"),
    ("ldt_sgemm", (P, 4, None, 4, None, P, 4, 0, 0, 0, 4, 4, 4, None), EARG, "sgemm: null pointer"),
    # -- samplers.hip
    ("ldt_sampler_step", (P, P, None, 0, P, None, P, None, 0, 0, 6, 0, 1, 1, 0, None), ESHAPE,
     "sampler_step: n and elem_offset must be multiples of 4 (n=6)"),
    ("ldt_sampler_step", (P, P, None, 0, P, None, P, None, 0, 0, 8, 2, 1, 1, 0, None), ESHAPE,
     "sampler_step: n and elem_offset must be multiples of 4 (n=8)"),
    ("ldt_sampler_step", (P, None, None, 0, P, None, P, None, 0, 0, 8, 0, 1, 1, 0, None), EARG, "sampler_step: null pointer"),
    ("ldt_sampler_step", (P, ODD, None, 0, P, None, P, None, 0, 0, 8, 0, 1, 1, 0, None), EALIGN, "sampler_step: buffers must be 16-byte aligned"),
    ("ldt_sampler_step", (P, P, None, 0, P, None, P, None, 0, 2, 8, 0, 1, 1, 0, None), EARG, "sampler_step: mode 2"),
    ("ldt_sampler_step_traj", (P, P, None, 0, P, None, ODD, P, None, 0, 0, 8, 0, 1, 1, 0, None), EALIGN,
     "sampler_step_traj: traj must be 16-byte aligned"),
    ("ldt_sampler_step_traj", (P, P, None, 0, P, None, P, P, None, 0, 0, 6, 0, 1, 1, 0, None), ESHAPE,
     "sampler_step: n and elem_offset must be multiples of 4 (n=6)"),
    ("ldt_sampler_step_traj", (P, None, None, 0, P, None, P, P, None, 0, 0, 8, 0, 1, 1, 0, None), EARG, "sampler_step: null pointer"),
    ("ldt_philox_normal", (None, 8, 0, 0, 1, None), EARG, "philox_normal: null pointer"),
    ("ldt_philox_normal", (P, 6, 0, 0, 1, None), ESHAPE, "philox_normal: n/offset % 4, 16-byte aligned"),
    ("ldt_philox_normal", (P, 8, 2, 0, 1, None), ESHAPE, "philox_normal: n/offset % 4, 16-byte aligned"),
    ("ldt_philox_normal", (ODD, 8, 0, 0, 1, None), ESHAPE, "philox_normal: n/offset % 4, 16-byte aligned"),
    # -- pointops.hip
    ("ldt_fps", (None, 1, 8, 4, 0, P, None), EARG, "fps: null pointer"),
    ("ldt_fps", (P, 1, 8, 4, 0, None, None), EARG, "fps: null pointer"),
    ("ldt_fps", (P, 1, 4, 5, 0, P, None), ESHAPE, "fps: B=1 n=4 m=5"),
    ("ldt_fps", (P, 0, 4, 2, 0, P, None), ESHAPE, "fps: B=0 n=4 m=2"),
    ("ldt_fps", (P, 1, 8193, 4, 0, P, None), ESHAPE, "fps: n=8193 > 8192 points per cloud not built"),
    ("ldt_knn", (P, None, 1, 8, 2, 4, P, None, None), EARG, "knn: null pointer"),
    ("ldt_knn", (P, P, 1, 4, 2, 5, P, None, None), ESHAPE, "knn: B=1 n=4 S=2 k=5"),
    ("ldt_knn", (P, P, 1, 8193, 2, 4, P, None, None), ESHAPE, "knn: n=8193 > 8192 points per cloud not built"),
    ("ldt_group_normalize", (P, P, P, P, P, P, None, 1, 8, 2, 4, 4, P, 16, 0, None, None), EARG, "group: null pointer"),
    ("ldt_group_normalize", (P, P, P, P, P, P, P, 1, 8, 2, 4, 4, P, 10, 0, None, None), ESHAPE, "group: bad shape"),
    ("ldt_group_normalize", (P, P, P, P, P, P, P, 1, 8, 2, 4, 4, P, 16, 1, None, None), EARG,
     "group: mode 1 ('center') needs the group-mean workspace"),
    ("ldt_group_normalize", (P, P, P, P, P, P, P, 1, 8, 2, 4, 4, P, 16, 2, P, None), EARG,
     "group: mode 1 ('center') needs the group-mean workspace"),
    ("ldt_norm_points", (P, 1, 8, None, None), EARG, "norm_points: null pointer"),
    ("ldt_norm_points", (P, 1, 1, P, None), ESHAPE, "norm_points: B=1 n=1"),
    ("ldt_mixture_seed", (P, P, P, None, 2, 4, 2, P, None), EARG, "mixture_seed: null pointer"),
    ("ldt_mixture_seed", (P, P, P, P, 9, 4, 2, P, None), ESHAPE, "mixture_seed: n_mix=9 (<= 8) D=4 rows=2"),
    ("ldt_gather_rows", (P, None, 1, 8, 2, 4, P, None), EARG, "gather_rows: null pointer"),
    ("ldt_gather_rows", (P, P, 1, 8, 2, 0, P, None), ESHAPE, "gather_rows: bad shape"),
    ("ldt_maxpool", (None, 0, 4, 2, 3, 4, P, None), EARG, "maxpool: null pointer"),
    ("ldt_maxpool", (P, 0, 3, 2, 3, 4, P, None), ESHAPE, "maxpool: bad shape"),
    ("ldt_chamfer", (P, P, 1, 4, 4, P, None, None), EARG, "chamfer: null pointer"),
    ("ldt_chamfer", (P, P, 1, 0, 4, P, P, None), ESHAPE, "chamfer: bad shape"),
    # -- actnorm.hip
    ("ldt_actnorm", (P, None, P, 2, 4, None), EARG, "actnorm: null pointer"),
    ("ldt_actnorm", (P, P, P, 0, 4, None), ESHAPE, "actnorm: bad shape"),
    ("ldt_actnorm_bwd", (None, P, P, 2, 4, P, P, P, None), EARG, "actnorm_bwd: null pointer (dlog_scale needs z)"),
    ("ldt_actnorm_bwd", (P, None, P, 2, 4, P, None, P, None), EARG, "actnorm_bwd: null pointer (dlog_scale needs z)"),
    ("ldt_actnorm_bwd", (P, P, P, 0, 4, P, P, P, None), EARG, "actnorm_bwd: B 0, per_sample 4"),
    ("ldt_actnorm_bwd", (P, P, P, 2, 0, P, P, P, None), EARG, "actnorm_bwd: B 2, per_sample 0"),
    ("ldt_actnorm_bwd", (P, P, P, 65535 * 512 + 1, 4, P, None, None, None), ESHAPE, "actnorm_bwd: B 33553921, per_sample 4"),
    # -- eval_loss.hip
    ("ldt_reparam", (P, None, P, 4, None, None, 2, 4, F, F, None), EARG, "reparam: null pointer"),
    ("ldt_reparam", (P, P, P, 3, None, None, 2, 4, F, F, None), ESHAPE, "reparam: bad shape"),
    ("ldt_reparam", (P, P, P, 4, P, None, 2, 4, F, F, None), EARG, "reparam: mu/logvar outputs go together"),
    # -- metrics.hip
    ("ldt_chamfer_pairwise", (P, P, 1, 1, 4, 4, None, None), EARG, "chamfer_pairwise: null pointer"),
    ("ldt_chamfer_pairwise", (P, P, 65536, 1, 4, 4, P, None), ESHAPE, "chamfer_pairwise: bad shape S=65536 R=1 n=4 m=4"),
    ("ldt_emd_approx", (P, None, 1, 1, 4, 4, 0, P, None), EARG, "emd_approx: null pointer"),
    ("ldt_emd_approx", (P, P, 1, 1, 0, 4, 0, P, None), ESHAPE, "emd_approx: bad shape"),
    ("ldt_emd_approx", (P, P, 2, 3, 4, 4, 0, P, None), ESHAPE, "emd_approx: batched mode pairs cloud b with cloud b (S=2 != R=3)"),
    ("ldt_emd_approx", (P, P, 2, 3, 4000, 4000, 1, P, None), ESHAPE, "emd_approx: n + m = 8000 points exceed the LDS-resident limit (7680)"),
    # -- grouper_mlp.hip
    ("ldt_grouper_mlp", (P, P, P, P, P, P, P, 1, 8, 2, 8, 128, None, P, P, P, P, None), EARG, "grouper_mlp: null pointer"),
    ("ldt_grouper_mlp", (P, P, P, P, P, P, P, 1, 8, 2, 8, 64, P, P, P, P, P, None), ESHAPE,
     "grouper_mlp: the fused kernel is built for 128 channels (got D=64)"),
    ("ldt_grouper_mlp", (P, P, P, P, P, P, P, 0, 8, 2, 8, 128, P, P, P, P, P, None), ESHAPE, "group_stats: bad shape"),
    # -- fused_mlp.hip
    ("ldt_ln_mlp_resid", (P, 64, 4, 64, None, None, None, None, None, 0, 0, P, None, P, P, None, 0, None), EARG, "ln_mlp: null pointer"),
    ("ldt_ln_mlp_resid", (P, 64, 0, 64, None, None, None, None, None, 0, 0, P, P, P, P, None, 0, None), ESHAPE, "ln_mlp: bad row count 0"),
    ("ldt_ln_mlp_resid", (P, 64, 4, 32, None, None, None, None, None, 0, 0, P, P, P, P, None, 0, None), ESHAPE,
     "ln_mlp: the fused kernel is built for 64 or 128 channels (got 32)"),
    ("ldt_ln_mlp_resid", (ODD, 64, 4, 64, None, None, None, None, None, 0, 0, P, P, P, P, None, 0, None), EALIGN,
     "ln_mlp: x rows must be 16-byte aligned"),
    ("ldt_ln_mlp_resid", (P, 64, 4, 64, P, None, None, None, None, 0, 0, P, P, P, P, None, 0, None), EARG,
     "ln_mlp: affine weight and bias go together"),
    ("ldt_ln_mlp_resid", (P, 64, 4, 64, None, None, None, None, None, 0, 0, P, P, P, P, ODD + 2, 64, None), EALIGN,
     "ln_mlp: bf16 mirror rows must be 8-byte aligned"),
    ("ldt_ln_mlp_resid_next", (P, 64, 4, 64, None, None, None, None, None, 0, 0, P, P, P, P, None, 0,
                               None, None, None, None, 0, 0, None, None, 64, P, 64, None), EARG, "ln_mlp_next: null pointer"),
    ("ldt_ln_mlp_resid_next", (P, 64, 4, 64, None, None, None, None, None, 0, 0, P, P, P, P, None, 0,
                               None, None, None, None, 0, 0, P, None, 32, P, 64, None), EARG,
     "ln_mlp: the follow-on LN + linear needs N % 64 == 0 and a 16-byte aligned weight, bias and bf16 output"),
    ("ldt_ln_mlp_resid_next", (P, 64, 4, 64, None, None, None, None, None, 0, 0, P, P, P, P, None, 0,
                               None, None, P, None, 0, 1, P, None, 64, P, 64, None), EARG,
     "ln_mlp: the follow-on LN + linear: shift and scale go together"),
    ("ldt_ln_linear", (P, 64, 4, 64, None, None, None, None, 0, 0, None, None, 64, P, 64, None), EARG, "ln_linear: null pointer"),
    ("ldt_ln_linear", (P, 64, 4, 64, None, None, None, None, 0, 0, P, None, 32, P, 64, None), ESHAPE, "ln_linear: N=32 must be a multiple of 64"),
    ("ldt_ln_linear", (P, 64, 4, 64, None, None, None, None, 0, 0, P, None, 64, P, 60, None), EALIGN, "ln_linear: rows must be 16-byte aligned"),
    ("ldt_ln_linear", (P, 64, 4, 64, None, None, ODD, P, 0, 1, P, None, 64, P, 64, None), EARG,
     "ln_linear: shift, scale and gate must be 16-byte aligned"),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name,args,status,text", CASES, ids=["%s-%d" % (c[0][4:], i) for i, c in enumerate(CASES)])
def test_entry_reports_status_and_message(lib, name, args, status, text):
    # a message left by an earlier call must not pass for this one: leave another op's first
    if name == "ldt_cast_pad_bf16":
        assert lib.ldt_sinusoid(None, None, None, 0, 0, None) == EARG and lib.ldt_last_error() == b"sinusoid: null pointer"
    else:
        assert lib.ldt_cast_pad_bf16(None, 0, None, 0, 0, 0, 0, None) == EARG and lib.ldt_last_error() == b"cast_pad: null pointer"
    rc = getattr(lib, name)(*args)
    print("%s -> %d %r" % (name, rc, lib.ldt_last_error()))
    assert rc == status
    assert lib.ldt_last_error().decode() == text


def test_every_moved_entry_is_covered():
    moved = {"ldt_cast_pad_bf16", "ldt_layernorm_modulate", "ldt_sinusoid", "ldt_sgemm", "ldt_sampler_step", "ldt_sampler_step_traj",
             "ldt_philox_normal", "ldt_fps", "ldt_knn", "ldt_group_normalize", "ldt_norm_points", "ldt_mixture_seed", "ldt_gather_rows",
             "ldt_maxpool", "ldt_chamfer", "ldt_actnorm", "ldt_actnorm_bwd", "ldt_reparam", "ldt_chamfer_pairwise", "ldt_emd_approx",
             "ldt_grouper_mlp", "ldt_ln_mlp_resid", "ldt_ln_mlp_resid_next", "ldt_ln_linear"}
    assert {c[0] for c in CASES} == moved
    for name in moved:                            # each with a null-pointer case and at least one further check
        kinds = {c[2] for c in CASES if c[0] == name}
        assert len([c for c in CASES if c[0] == name]) >= 2 and EARG in kinds, name
